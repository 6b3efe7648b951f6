"""libelas' Delaunay triangulation of the support points (Elas::computeDelaunayTriangulation, elas.cpp:492-556, i.e. Triangle's
triangulate("zQB")) as the product computes it on the host (plvs_amd/csrc/elas_delaunay.hpp, plvs_hip_elas_triangulate):
the same triangles, in the same order, each with its corners in the same order — computeDisparity rasterises them in
that order.  CPU only: the library loads without a GPU.

The reference's own triangles come from the compiled reference pipeline (oracle/_ref/libelas_ref.so, tests/elas_ref.py):
every computeDisparity call it makes hands over the support list and the triangles it triangulated."""
import lzma
import os
import shutil

import numpy as np
import pytest

from plvs_amd.elas import ElasGPU, SUPPORT_PT
from tests import elas_ref, oracle_lib
from tests.pgm import read_pgm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
needs_ref = pytest.mark.skipif(not elas_ref.available(), reason="needs oracle/_ref/libelas_ref.so (built where /root/reference is)")
ROBOTICS, MIDDLEBURY = 1, 3        # elas_ref's `plvs`: bit 0 postprocess_only_left, bit 1 the MIDDLEBURY set (add_corners)


def corners(tri):
    return np.stack([tri["c1"], tri["c2"], tri["c3"]], -1).astype(np.int32)


def vertices(support, right_image):
    s = np.ascontiguousarray(support).view(SUPPORT_PT).reshape(-1)
    return s["u"] - (s["d"] if right_image else 0), s["v"]


def has_duplicates(support, right_image):
    x, y = vertices(support, right_image)
    return len(set(zip(x.tolist(), y.tolist()))) < len(x)


def read_xz_pgm(path):       # (binary P5 with comment lines, which GIMP writes into some of the tree's files)
    data = lzma.decompress(open(path, "rb").read())
    tokens, pos = [], 0
    while len(tokens) < 4:
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
            continue
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        tokens.append(data[pos:end])
        pos = end
    assert tokens[0] == b"P5" and int(tokens[3]) == 255
    w, h = int(tokens[1]), int(tokens[2])
    return np.frombuffer(data, np.uint8, w * h, pos + 1).reshape(h, w).copy()


def pair(name):
    if name.startswith("urban1"):
        left = read_pgm(os.path.join(GOLDEN, "urban1_1241x376.pgm"))
        right = read_pgm(os.path.join(GOLDEN, "urban1_right_1241x376.pgm"))
        w, h = {"urban1": (1241, 376), "urban1_640": (640, 300), "urban1_333": (333, 201)}[name]
        return np.ascontiguousarray(left[:h, :w]), np.ascontiguousarray(right[:h, :w])
    tree = os.path.join(GOLDEN, "libelas")
    return read_xz_pgm(os.path.join(tree, f"{name}_left.pgm.xz")), read_xz_pgm(os.path.join(tree, f"{name}_right.pgm.xz"))


def product(support, right_image):
    return corners(ElasGPU.triangulate(support, right_image))


def check_calls(calls, triangulate=product):
    """Every recorded computeDisparity call: the product's (or another build's) triangles equal the reference's."""
    for c in calls:
        got = triangulate(c["support"], c["right_image"])
        want = corners(c["tri"])
        assert got.shape == want.shape, (c["right_image"], len(c["support"]), got.shape, want.shape)
        assert np.array_equal(got, want), (c["right_image"], len(c["support"]), int(np.argmax((got != want).any(-1))))


# ------------------------------------------------------------------ 1. the committed capture (no reference, no GPU)
def test_committed_capture_triangles():
    """tests/golden/elas_capture.npz: the support list and the triangles the reference handed to both computeDisparity
    calls of one pair (urban1, 256 x 128)."""
    z = np.load(os.path.join(GOLDEN, "elas_capture.npz"))
    for i in range(int(z["n_disparity_calls"])):
        sup = np.ascontiguousarray(z[f"d{i}_support"]).view(SUPPORT_PT).reshape(-1)
        want = np.ascontiguousarray(z[f"d{i}_tri"][:, :3]).view(np.int32)
        tri = ElasGPU.triangulate(sup, int(z[f"d{i}_right_image"]))
        assert np.array_equal(corners(tri), want)
        for k in ("t1a", "t1b", "t1c", "t2a", "t2b", "t2c"):
            assert not tri[k].any()


# ------------------------------------------------------------------ 2. the reference pipeline on real pairs
PAIRS = ["urban1", "urban1_640", "urban1_333", "cones", "aloe", "raindeer", "urban3"]


@needs_ref
@pytest.mark.parametrize("name", PAIRS)
@pytest.mark.parametrize("subsampling", [False, True])
@pytest.mark.parametrize("setting", [ROBOTICS, MIDDLEBURY])
def test_reference_pipeline_triangles(name, subsampling, setting):
    """Left and right triangulations of every pair the tree ships (urban1 at three sizes), with and without subsampling,
    in the ROBOTICS and the MIDDLEBURY setting (add_corners): the reference's triangles, in order, corner by corner."""
    left, right = pair(name)
    calls, _, _ = elas_ref.capture(left, right, subsampling=subsampling, plvs=setting)
    assert sorted(c["right_image"] for c in calls) == [0, 1]
    check_calls(calls)


# ------------------------------------------------------------------ 3. seeded candidate grids through the real pipeline
def fuzz_grid(seed, shape):
    """One seeded D_can (int16, -1 = no candidate; row / column 0 stay 0 as the reference's calloc leaves them) of one of
    six kinds: sparse, medium or dense validity with nearby disparities, constant patches, rows whose right-image
    vertices u - d collide, a single row or column."""
    rng = np.random.default_rng(seed)
    h, w = shape
    kind = seed % 6
    D = np.full(shape, -1, np.int32)
    if kind in (0, 1, 2):
        density = (0.15, 0.5, 0.95)[kind]
        base = rng.integers(0, 60)
        smooth = base + np.cumsum(rng.integers(-1, 2, shape), axis=1) // 3
        valid = rng.random(shape) < density
        D[valid] = np.clip(smooth + rng.integers(-3, 4, shape), 0, 255)[valid]
    elif kind == 3:
        for _ in range(rng.integers(2, 8)):
            v0, u0 = rng.integers(0, h), rng.integers(0, w)
            D[v0:v0 + rng.integers(3, h), u0:u0 + rng.integers(3, w)] = rng.integers(0, 80)
        D[rng.random(shape) < 0.05] = -1
    elif kind == 4:
        # d = 5 * (u_can - c) (+ a jitter of 0 or 5): on a row, every point of a band lands on u - d = 5 c
        step = 5
        u = np.arange(w)[None, :]
        c = rng.integers(0, w // 2, (h, 1))
        d = step * (u - c) + step * rng.integers(0, 2, shape)
        valid = (d >= 0) & (d <= 255) & (rng.random(shape) < 0.9)
        D[valid] = d[valid]
    else:
        if rng.random() < 0.5:
            r = rng.integers(1, h)
            D[r, :] = np.clip(rng.integers(20, 40) + rng.integers(-2, 3, w), 0, 255)
        else:
            col = rng.integers(1, w)
            D[:, col] = np.clip(rng.integers(20, 40) + rng.integers(-2, 3, h), 0, 255)
    D[0, :] = 0
    D[:, 0] = 0
    return D.astype(np.int16)


FUZZ_CASES = 240


def fuzz_calls(seed, left, right):
    """The reference pipeline on (left, right) with fuzz_grid(seed) as its candidate grid: its computeDisparity calls."""
    calls = []

    def record(a):
        calls.append(dict(support=a["support"], tri=a["tri"], right_image=a["right_image"]))
        return np.zeros(a["height"] // 2 * (a["width"] // 2) if a["subsampling"] else a["height"] * a["width"], np.float32)

    def candidates(a):
        h, w = a["height"], a["width"]
        step = 5 + (5 % 2 if a["subsampling"] else 0)
        return fuzz_grid(seed, (-(-h // step), -(-w // step)))

    elas_ref.run_with(left, right, record, None, subsampling=bool(seed % 4 == 3),
                      plvs=MIDDLEBURY if seed % 2 else ROBOTICS, support_candidates=candidates)
    return calls


@needs_ref
def test_fuzzed_candidate_grids_through_the_reference_pipeline():
    """240 seeded candidate grids injected into the reference's own filters (sparse / medium / dense validity, constant
    patches, colliding u - d on a row, single rows and columns; ROBOTICS and MIDDLEBURY, subsampling on for a quarter):
    every triangulation the reference then makes, left and right, is the product's."""
    left, right = pair("urban1_333")
    n_calls = n_dup = n_empty = 0
    for seed in range(FUZZ_CASES):
        calls = fuzz_calls(seed, left, right)
        check_calls(calls)
        n_calls += len(calls)
        n_dup += any(has_duplicates(c["support"], c["right_image"]) for c in calls)
        n_empty += any(len(c["tri"]) == 0 for c in calls)
    print(f"\n{FUZZ_CASES} grids, {n_calls} triangulations: {n_dup} cases with duplicate vertices, "
          f"{n_empty} with no triangle (collinear)")
    assert n_calls >= FUZZ_CASES
    assert n_dup >= 20, "the fuzz no longer reaches duplicate vertices"


# ------------------------------------------------------------------ 4. the same header under other compilers
def host_triangulate(stem):
    import ctypes
    src = os.path.join(ROOT, "tests", "host", "elas_delaunay_host.cpp")
    hdr = os.path.join(ROOT, "plvs_amd", "csrc", "elas_delaunay.hpp")
    lib = ctypes.CDLL(oracle_lib._host_build(stem, src, [hdr]))
    lib.hostdt_triangulate.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]

    def triangulate(support, right_image):
        sup = np.ascontiguousarray(np.ascontiguousarray(support).view(np.int32).reshape(-1, 3))
        out = np.zeros((2 * len(sup) + 2, 3), np.int32)
        n = lib.hostdt_triangulate(sup.ctypes.data, len(sup), int(right_image), out.ctypes.data, len(out))
        return out[:n]
    return triangulate


def random_supports(count):
    """Seeded point sets the pipeline does not make: many duplicates, collinear runs, negative u - d."""
    for seed in range(count):
        rng = np.random.default_rng(1000 + seed)
        n = int(rng.integers(3, 400))
        span = int(rng.choice([3, 10, 60, 400]))
        s = np.zeros(n, SUPPORT_PT)
        s["u"] = 5 * rng.integers(0, span, n)
        s["v"] = 5 * rng.integers(0, span // 2 + 1, n) if seed % 5 else 5 * (seed % 7)
        s["d"] = 5 * rng.integers(0, 8, n)
        yield s


@pytest.mark.parametrize("compiler", ["g++", "rocm-clang"])
def test_host_builds_agree_with_the_library(compiler, monkeypatch):
    """elas_delaunay.hpp through g++ -O2 and (where present) ROCm clang -O3 gives what the library's build gives: on the
    committed capture, seeded point sets full of duplicates and collinear runs and, where the reference is built, the
    reference pipeline's own support lists."""
    if compiler == "rocm-clang":
        if not os.path.exists(oracle_lib.ROCM_CLANG):
            pytest.skip("no ROCm clang on this machine")
        monkeypatch.setenv("PLVS_HOST_CXX", "rocm-clang")
    elif shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    host = host_triangulate("libhostdelaunay")
    z = np.load(os.path.join(GOLDEN, "elas_capture.npz"))
    sets = [(np.ascontiguousarray(z[f"d{i}_support"]).view(SUPPORT_PT).reshape(-1), int(z[f"d{i}_right_image"]))
            for i in range(int(z["n_disparity_calls"]))]
    sets += [(s, k % 2) for k, s in enumerate(random_supports(300))]
    n_empty = 0
    for sup, r in sets:
        got = host(sup, r)
        assert np.array_equal(got, product(sup, r))
        n_empty += len(got) == 0
    assert n_empty > 0                                     # (collinear sets are among them)
    if elas_ref.available():
        left, right = pair("urban1_640")
        calls, _, _ = elas_ref.capture(left, right, subsampling=False, plvs=MIDDLEBURY)
        check_calls(calls, host)
        for seed in range(24):
            check_calls(fuzz_calls(seed, *pair("urban1_333")), host)


def test_errors():
    from plvs_amd import _lib
    with pytest.raises(_lib.PlvsHipError) as e:
        ElasGPU.triangulate(np.zeros(2, SUPPORT_PT), 0)
    assert e.value.code == _lib.PLVS_ERR_EMPTY
    s = np.zeros(40, SUPPORT_PT)
    s["u"], s["v"] = 5 * (np.arange(40) % 8), 5 * (np.arange(40) // 8)
    tri = ElasGPU.triangulate(s, 0)
    assert len(tri) == 2 * (8 - 1) * (5 - 1)               # a 8 x 5 lattice: two triangles per cell
    import ctypes
    n = ctypes.c_int()
    out = np.zeros(3, ElasGPU.triangulate(s, 0).dtype)
    rc = _lib.lib.plvs_hip_elas_triangulate(_lib.np_ptr(s), len(s), 0, _lib.np_ptr(out), len(out), ctypes.byref(n))
    assert rc == _lib.PLVS_ERR_CAPACITY and n.value == len(tri)
