"""The dense-stereo (semi-global matching) case table.  Run three ways over the SAME table:
  scripts/make_sgm_golden.py            libsgm's own CUDA kernels, compiled for the CPU and executed by the stand-in of
                                        oracle/ref/cuda_shim/ (oracle/_ref/libsgm_ref.so) -> tests/golden/sgm_reference_digests.json
  tests/test_oracle_pinned_sgm.py, CPU  oracle/sgm.c equals the compiled reference array for array (where oracle/_ref exists),
                                        and reproduces the file on its own (everywhere)
  tests/test_sgm.py, GPU                the HIP path equals the oracle array for array and reproduces the file
A runner is  fn(left [h, w] u8, right [h, w] u8, P1, P2, uniqueness) -> dict of the STAGES' arrays.

Shapes are w x h, the smallest at which each mechanism can fail: 16 x 16 is the minimum create() accepts (every
right[x - d] clipped, one block of the consistency grid); 16 x 80 is taller than wide (most of an oblique path lies
outside); 63 / 64 / 65 wide are either side of the 64 disparities = the wave width, with neither side a multiple of 4
(the median's two variants) or 16 (the consistency grid); 130 x 67 has more than one block of every kernel.
No case has left the table: the compiled reference is defined on all of them (see tests/test_oracle_pinned_sgm.py)."""
import hashlib

import numpy as np

from tests.oracle_lib import golden

STAGES = (["census_left", "census_right"] + [f"path{i}" for i in range(8)] +
          ["raw_left", "raw_right", "median_left", "median_right", "final"])
DEFAULT = (10, 120, 0.95)
PARAMS = [DEFAULT, (0, 0, 1.0), (7, 60, 0.9), (224, 224, 0.5), (1, 224, 1.0), (10, 120, 0.0), (10, 120, 2.0)]
REAL_SHAPES = [(16, 16), (16, 80), (80, 16), (63, 17), (64, 19), (65, 33), (130, 67), (64, 48), (333, 181)]
SYNTHETIC = ["noise", "constant", "zeros", "all255", "stripes", "swapped"]
# where the real crops come from in the committed urban1 pair (x0, y0); the two older cases keep theirs
ORIGIN = {(333, 181): (500, 100)}


def _case(kind, w, h, params=DEFAULT, **kw):
    p1, p2, u = params
    cid = f"{kind}_{w}x{h}" + ("" if params == DEFAULT else f"_p{p1}_{p2}_u{u}")
    return dict(id=cid, kind=kind, width=w, height=h, P1=p1, P2=p2, uniqueness=u, **kw)


def _table():
    cases = [_case("real", w, h) for w, h in REAL_SHAPES]
    cases += [_case(kind, w, h) for w, h in ((65, 33), (16, 80)) for kind in SYNTHETIC]
    cases += [_case(kind, 65, 33, p) for p in PARAMS[1:] for kind in ("real", "stripes")]
    return cases


CASES = _table()
# the KITTI-shaped pair: in the golden file only (minutes under emulation); tests/test_sgm.py's GPU case reproduces it
KITTI = _case("real", 1240, 376, origin=(0, 0))
# too slow under emulation for the CPU suite's oracle-against-reference half (measured times: the test's docstring);
# their digests are in the golden file, so the oracle and the HIP path are still held to the reference on them
EMULATED_IN_SUITE = [c for c in CASES if (c["width"], c["height"]) != (333, 181)]


def inputs(case):
    w, h, kind = case["width"], case["height"], case["kind"]
    if kind in ("real", "swapped"):
        x0, y0 = case.get("origin", ORIGIN.get((w, h), (300, 200)))
        left, right = (np.ascontiguousarray(golden(f)[y0:y0 + h, x0:x0 + w])
                       for f in ("urban1_1241x376.pgm", "urban1_right_1241x376.pgm"))
        return (right, left) if kind == "swapped" else (left, right)      # swapped: no positive disparity fits
    if kind == "noise":                # independent uniform noise: the largest costs, sums near 8 * (P2 + 31)
        rng = np.random.default_rng(1000 * w + h)
        return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "stripes":              # period 8: equal costs at several disparities, both branches after the uniqueness test
        row = np.where(np.arange(w) % 8 < 4, 64, 192).astype(np.uint8)
        img = np.ascontiguousarray(np.broadcast_to(row, (h, w)))
        return img, img.copy()
    value = {"constant": 128, "zeros": 0, "all255": 255}[kind]
    img = np.full((h, w), value, np.uint8)
    return img, img.copy()


def split_paths(st):
    """A dict with "paths" [8, h, w, 64] -> the same with path0 .. path7."""
    out = {k: v for k, v in st.items() if k != "paths"}
    for i in range(8):
        out[f"path{i}"] = st["paths"][i]
    return out


def digests(st):
    return {k: hashlib.sha256(np.ascontiguousarray(st[k]).tobytes()).hexdigest() for k in STAGES}


def run(fn, cases):
    out = {}
    for c in cases:
        left, right = inputs(c)
        out[c["id"]] = digests(fn(left, right, c["P1"], c["P2"], c["uniqueness"]))
    return out


def oracle_runner(oracle):
    def fn(left, right, p1, p2, u):
        disp, st = oracle.sgm(left, right, p1, p2, u, stages=True)
        st = split_paths(st)
        st["final"] = disp
        return st
    return fn
