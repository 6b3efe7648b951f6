"""oracle/sgm.c pinned by libsgm's own kernels: Thirdparty/libsgm/src/*.cu and stereo_sgm.cpp compiled
for the CPU where they lie, against the CUDA stand-in of oracle/ref/cuda_shim/ that EXECUTES a launch on the host
(oracle/ref/Makefile -> oracle/_ref/libsgm_ref.so; only the <<<...>>> launch expressions are rewritten, at build time).

  where oracle/_ref/libsgm_ref.so exists
       the oracle equals the compiled reference stage by stage, byte for byte — both census images, the eight path
       volumes one by one, raw / median-filtered left and right disparity, the final image — on every case of
       tests/sgm_golden_scenario.py but 333 x 181 (below); the reference's outputs are equal between an allocation fill
       of 0x00 and of 0xFF (it reads no memory it never wrote, given the one pin of oracle/ref/sgm_zero_malloc.h); the whole
       sgm::StereoSGM::execute gives the stages' final image.
  everywhere
       the oracle alone reproduces tests/golden/sgm_reference_digests.json (scripts/make_sgm_golden.py: a sha256 per stage
       and case, made by the compiled reference; with 333 x 181 and the KITTI-shaped 1240 x 376 pair);
       the stand-in itself: each shuffle kind at widths 8 and 32 against the table of CUDA's programming guide, a
       __syncthreads exchange between two warps, warps and half-warps that return early, a shuffle from a lane that has
       left (the process stops), a source lane outside the mask (the fill pattern), the packed-byte intrinsics against a
       per-byte loop, the allocation fill.

Time of the compiled reference under emulation, one run of the stages entry, measured where oracle/_ref is built
(scripts/make_sgm_golden.py prints them; the oracle takes under 0.1 s on each):
  16 x 16 0.01 s   16 x 80 0.05 s   80 x 16 0.04 s   63 x 17 0.03 s   64 x 19 0.04 s   65 x 33 0.07 s   64 x 48 0.10 s
  130 x 67 0.30 s   333 x 181 1.9 s   1240 x 376 14.5 s
A case costs three runs (two fills and the whole execute), computed once and shared by the tests of the case.  With
every shape up to 130 x 67 the file takes 8.5 s (test_oracle_pinned_elas.py 1.7 s; the other pinned files 1.4 to 16 s);
333 x 181 would add 6 s and 1240 x 376 three quarters of a minute, so those two are in the golden script only, where the
oracle and the HIP path are still held to the reference's digests on them."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import oracle_lib
from tests import sgm_golden_scenario as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libsgm_ref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sgm_reference_digests.json")
_i, _f, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


@functools.lru_cache(None)
def _ref():
    lib = ctypes.CDLL(REF)
    lib.sgm_ref_set_fill.argtypes = [_i]
    lib.sgm_ref_undefined_shuffles.restype = ctypes.c_ulong
    lib.sgm_ref_execute.argtypes = [_vp, _vp, _i, _i, _i, _i, _f, _vp]
    lib.sgm_ref_stages.argtypes = [_vp, _vp, _i, _i, _i, _i, _f] + [_vp] * 8
    return lib


def ref_stages(left, right, p1=10, p2=120, uniqueness=0.95, fill=0):
    """The compiled reference, stage by stage -> dict of S.STAGES' arrays."""
    lib = _ref()
    h, w = left.shape
    left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
    st = dict(census_left=np.zeros((h, w), np.uint32), census_right=np.zeros((h, w), np.uint32),
              paths=np.zeros((8, h, w, 64), np.uint8))
    for k in ("raw_left", "raw_right", "median_left", "median_right", "final"):
        st[k] = np.zeros((h, w), np.uint8)
    lib.sgm_ref_set_fill(fill)
    lib.sgm_ref_reset_counters()
    lib.sgm_ref_stages(left.ctypes.data, right.ctypes.data, w, h, p1, p2, uniqueness,
                       *[st[k].ctypes.data for k in ("census_left", "census_right", "paths", "raw_left", "raw_right",
                                                     "median_left", "median_right", "final")])
    lib.sgm_ref_set_fill(0)
    return S.split_paths(st)


def ref_execute(left, right, p1=10, p2=120, uniqueness=0.95, fill=0):
    """The compiled reference's whole sgm::StereoSGM(w, h, 64, 8, 8, HOST2HOST, Parameters(...))::execute."""
    lib = _ref()
    h, w = left.shape
    left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
    out = np.zeros((h, w), np.uint8)
    lib.sgm_ref_set_fill(fill)
    lib.sgm_ref_execute(left.ctypes.data, right.ctypes.data, w, h, p1, p2, uniqueness, out.ctypes.data)
    lib.sgm_ref_set_fill(0)
    return out


@functools.lru_cache(None)
def _reference_of(case_id):
    """One case through the compiled reference, computed once for the tests below: (stages with fill 0x00, stages with
    fill 0xFF, the whole execute with fill 0xFF)."""
    c = next(c for c in S.CASES if c["id"] == case_id)
    left, right = S.inputs(c)
    args = (left, right, c["P1"], c["P2"], c["uniqueness"])
    return ref_stages(*args, fill=0x00), ref_stages(*args, fill=0xFF), ref_execute(*args, fill=0xFF)


needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/libsgm_ref.so is built where /root/reference exists")
_suite = pytest.mark.parametrize("case", S.EMULATED_IN_SUITE, ids=[c["id"] for c in S.EMULATED_IN_SUITE])


@needs_ref
@_suite
def test_oracle_equals_the_compiled_reference(oracle, case):
    want = _reference_of(case["id"])[0]
    left, right = S.inputs(case)
    got = S.oracle_runner(oracle)(left, right, case["P1"], case["P2"], case["uniqueness"])
    for k in S.STAGES:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


@needs_ref
@_suite
def test_reference_does_not_depend_on_memory_it_never_wrote(case):
    """Allocations filled with 0x00 against 0xFF (and the shuffles CUDA leaves undefined returning the same byte)."""
    zero, ones, whole = _reference_of(case["id"])
    for k in S.STAGES:
        assert np.array_equal(zero[k], ones[k]), k
    assert np.array_equal(whole, zero["final"])          # StereoSGM::execute end to end = the stages one by one


def test_the_table_has_every_case_the_pin_names():
    ids = [c["id"] for c in S.CASES]
    assert len(ids) == len(set(ids)) == 9 + 12 + 12
    assert len(S.EMULATED_IN_SUITE) == len(ids) - 1


def test_oracle_reproduces_the_reference_made_digests(oracle):
    with open(GOLDEN) as f:
        want = json.load(f)["cases"]
    cases = S.CASES + [S.KITTI]
    assert sorted(want) == sorted(c["id"] for c in cases)
    got = S.run(S.oracle_runner(oracle), cases)
    for cid in want:
        for k in S.STAGES:
            assert got[cid][k] == want[cid][k], (cid, k)


# ---------------------------------------------------------------- the stand-in's own checks
@pytest.fixture(scope="module")
def shim():
    return oracle_lib.load_hostcudashim()


def _cuda_shuffle_table(kind, lane, arg, width):
    """CUDA C++ programming guide, "Warp Shuffle Functions", spelled out on its own: the source lane of `lane`."""
    first = lane - lane % width
    if kind == 0:                                   # __shfl_sync: srcLane modulo width, inside the lane's segment
        return first + arg % width
    if kind == 1:                                   # up: the lowest `delta` lanes of a segment are unchanged
        return lane if lane - arg < first else lane - arg
    if kind == 2:                                   # down: the highest `delta` lanes of a segment are unchanged
        return lane if lane + arg > first + width - 1 else lane + arg
    src = lane ^ arg                                # xor: an earlier segment may be read, a later one not
    return lane if src > first + width - 1 else src


@pytest.mark.parametrize("width", [8, 32])
@pytest.mark.parametrize("kind,args", [(0, [0, 3, 13, 31]), (1, [0, 1, 3, 9]), (2, [0, 1, 3, 9]), (3, [1, 4, 8, 16, 31])],
                         ids=["idx", "up", "down", "xor"])
def test_shim_shuffles_follow_cudas_table(shim, kind, args, width):
    shim.cuda_shim_reset_counters()
    for arg in args:
        out = np.zeros(128, np.uint32)
        shim.shimtest_shfl(out.ctypes.data, kind, arg, width)
        t = np.arange(128)
        lane, warp = t % 32, t % 64 // 32
        want = np.array([_cuda_shuffle_table(kind, int(l), arg, width) for l in lane]) + 100 * (warp + 1)
        assert np.array_equal(out, want), (kind, arg, width)
    assert shim.cuda_shim_undefined_shuffles() == 0


def test_shim_syncthreads_orders_an_exchange_between_two_warps(shim):
    out = np.zeros(192, np.uint32)
    shim.shimtest_exchange(out.ctypes.data)
    t = np.arange(64)
    for b in range(3):
        first = 1000 * (b + 1) + (t + 32) % 64                     # what thread t read in the first round
        assert np.array_equal(out[64 * b:64 * b + 64], 2 * first[(t + 33) % 64])


def test_shim_lets_warps_and_half_warps_return_early(shim):
    out = np.zeros(96, np.uint32)
    shim.shimtest_early_exit(out.ctypes.data)
    lane = np.arange(32)
    assert (out[16:64] == 7).all()                                                   # those that returned
    assert np.array_equal(out[:16], 65 + lane[:16])                                  # warp 0 reads warp 2's values
    down = np.where(lane % 16 == 15, 15, lane % 16 + 1)                              # __shfl_down by 1, width 16
    assert np.array_equal(out[64:], down + 1)


def test_shim_stops_on_a_shuffle_from_a_lane_that_has_left(shim):
    """No made-up value: the process is stopped, with the kernel and the lane in the message (a child process)."""
    code = ("import numpy as np; from tests import oracle_lib; lib = oracle_lib.load_hostcudashim(); "
            "out = np.zeros(32, np.uint32); lib.shimtest_dead_lane(out.ctypes.data); print('survived')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == -6 and "survived" not in r.stdout
    assert "dead_lane_kernel" in r.stderr and "lane" in r.stderr and "left the kernel" in r.stderr


def test_shim_marks_what_cuda_leaves_undefined(shim):
    """A source lane outside the mask (libsgm: every subgroup's first lane) gets the fill byte, and is counted; a fresh
    allocation holds the fill byte."""
    for fill in (0x00, 0xFF, 0x5A):
        shim.cuda_shim_set_fill(fill)
        shim.cuda_shim_reset_counters()
        out = np.zeros(32, np.uint32)
        shim.shimtest_outside_mask(out.ctypes.data)
        shim.cuda_shim_set_fill(0)
        lane = np.arange(32)
        want = np.where(lane == 0, 1, np.where(lane % 8 == 0, fill * 0x01010101, lane))
        assert np.array_equal(out, want)
        assert shim.cuda_shim_undefined_shuffles() == 3
        assert shim.shimtest_malloc_byte(fill) == fill * 0x0101


def test_shim_packed_intrinsics_equal_a_per_lane_loop(shim):
    edge8 = [0x00, 0x01, 0x7f, 0x80, 0xfe, 0xff]
    edge16 = [0x0000, 0x0001, 0x00ff, 0x0100, 0x7fff, 0x8000, 0xfffe, 0xffff]
    a, b = [], []
    for x in edge8:                     # every pair of boundary bytes, in each of the four byte positions, among
        for y in edge8:                 # other bytes that compare the other way round
            for pos in range(4):
                a.append(sum((x if p == pos else y) << 8 * p for p in range(4)))
                b.append(sum((y if p == pos else x) << 8 * p for p in range(4)))
    for x in edge16:
        for y in edge16:
            for pos in range(2):
                a.append(sum((x if p == pos else y) << 16 * p for p in range(2)))
                b.append(sum((y if p == pos else x) << 16 * p for p in range(2)))
    rng = np.random.default_rng(3)
    a = np.concatenate([np.array(a, np.uint32), rng.integers(0, 2 ** 32, 300, dtype=np.uint32)])
    b = np.concatenate([np.array(b, np.uint32), rng.integers(0, 2 ** 32, 300, dtype=np.uint32)])
    n = len(a)
    out = np.zeros((6, n), np.uint32)
    shim.shimtest_packed(a.ctypes.data, b.ctypes.data, out.ctypes.data, n)

    def lanes(bits, f):
        r = np.zeros(n, np.uint64)
        for s in range(0, 32, bits):
            m = (1 << bits) - 1
            x, y = (a.astype(np.uint64) >> s) & m, (b.astype(np.uint64) >> s) & m
            r |= (f(x, y, m).astype(np.uint64) & m) << s
        return r.astype(np.uint32)
    gt = lambda x, y, m: np.where(x > y, m, 0)                                      # noqa: E731
    for row, (bits, f) in enumerate([(16, gt), (8, gt), (16, lambda x, y, m: np.minimum(x, y)), (8, lambda x, y, m: np.minimum(x, y)),
                                     (16, lambda x, y, m: np.maximum(x, y)), (8, lambda x, y, m: np.maximum(x, y))]):
        assert np.array_equal(out[row], lanes(bits, f)), row
