#!/usr/bin/env python3
"""Golden digests of dense stereo by semi-global matching made by the REFERENCE ITSELF: libsgm's CUDA kernels and
stereo_sgm.cpp (/root/reference/Thirdparty/libsgm/src), compiled here for the CPU against the CUDA stand-in of
oracle/ref/cuda_shim/ (oracle/ref/Makefile, sgm_ref_wrap.cpp -> oracle/_ref/libsgm_ref.so), run over the case table of
tests/sgm_golden_scenario.py plus the KITTI-shaped 1240 x 376 pair (too slow under emulation for the suite); a sha256 per
stage and case goes to tests/golden/sgm_reference_digests.json.  Dev-time tool (needs the compiled reference);
tests/test_oracle_pinned_sgm.py checks the oracle (CPU) and tests/test_sgm.py the HIP path (GPU) against the file."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import sgm_golden_scenario as S                      # noqa: E402
from tests.test_oracle_pinned_sgm import ref_stages             # noqa: E402


def main():
    times = {}

    def timed(left, right, p1, p2, u):
        t = time.time()
        st = ref_stages(left, right, p1, p2, u)
        times[f"{left.shape[1]}x{left.shape[0]}"] = round(time.time() - t, 2)
        return st
    out = dict(what="sha256 digests of the stages of sgm::StereoSGM(w, h, 64, 8, 8, ...)::execute — census left / right, the eight "
                    "path volumes in PathAggregation::get_output()'s order, raw and median-filtered left / right disparity, the "
                    "final image — produced by libsgm's own kernels compiled for the CPU (see this script)",
               cases=S.run(timed, S.CASES + [S.KITTI]))
    path = os.path.join(ROOT, "tests", "golden", "sgm_reference_digests.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(path, len(out["cases"]), "cases; seconds per shape under emulation:", times)


if __name__ == "__main__":
    main()
