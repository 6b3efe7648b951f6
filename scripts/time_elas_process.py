"""Times ElasGPU.process (Elas::process in one call) per 1241 x 376 pair (tests/golden/urban1*), with and without
subsampling: 5 warm-up pairs, then 50 timed on a host clock around calls that end in the D1 / D2 download; the host
triangulation of the pair is timed apart (plvs_hip_elas_triangulate on the same support list).  One JSON line per setting.
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python scripts/time_elas_process.py`."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from plvs_amd.elas import ElasGPU  # noqa: E402
from tests.pgm import read_pgm  # noqa: E402


def main():
    left = read_pgm(os.path.join(ROOT, "tests", "golden", "urban1_1241x376.pgm"))
    right = read_pgm(os.path.join(ROOT, "tests", "golden", "urban1_right_1241x376.pgm"))
    h, w = left.shape
    for subsampling in (False, True):
        e = ElasGPU(ElasGPU.Parameters(subsampling=subsampling))
        for _ in range(5):
            e.process(left, right)
        ts = []
        for _ in range(50):
            t0 = time.perf_counter()
            e.process(left, right)
            ts.append(time.perf_counter() - t0)
        e.setImages(left, right)
        sup = e.supportPoints(e.supportCandidates(None, None, w, h), w, h)
        tt = []
        for _ in range(50):
            t0 = time.perf_counter()
            ElasGPU.triangulate(sup, 0)
            ElasGPU.triangulate(sup, 1)
            tt.append(time.perf_counter() - t0)
        ts, tt = np.array(ts) * 1e3, np.array(tt) * 1e3
        print(json.dumps(dict(pair="urban1 1241x376", subsampling=subsampling, support_points=int(len(sup)),
                              process_ms_median=round(float(np.median(ts)), 3),
                              process_ms_p10_p90=[round(float(np.percentile(ts, 10)), 3), round(float(np.percentile(ts, 90)), 3)],
                              triangulate_both_ms_median=round(float(np.median(tt)), 3),
                              triangulate_both_ms_p10_p90=[round(float(np.percentile(tt, 10)), 3),
                                                           round(float(np.percentile(tt, 90)), 3)])), flush=True)
        e.close()


if __name__ == "__main__":
    main()
