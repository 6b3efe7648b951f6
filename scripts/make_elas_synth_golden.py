#!/usr/bin/env python3
"""Writes tests/golden/elas_synth_reference_digests.json: sha256 of what the COMPILED reference's removeSmallSegments,
gapInterpolation, leftRightConsistencyCheck and adaptiveMean make of the synthetic cases of tests/elas_synth.py — per case,
per reference parameter set (0: ROBOTICS, 2: MIDDLEBURY; "mean": adaptiveMean called directly) and per map of the run.  Run
where oracle/_ref/libelas_ref.so exists; tests/test_elas_synth_reference.py holds the oracle to the digests where it does not.
(MIDDLEBURY's gap cases record the pipeline's median-filtered result: see test_oracle_equals_the_compiled_reference.)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_elas_synth_reference as T  # noqa: E402

out = {}
for name in T.REACHABLE:
    case = T.BY_NAME[name]
    out[name] = {str(mode): [T.digest(w) for w in T.reference_results(case, mode)] for mode in T.modes(case)}
for name in T.MEAN_REF:
    out[name] = {"mean": [T.digest(T.reference_mean(T.BY_NAME[name]))]}
with open(T.DIGESTS, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print(T.DIGESTS, os.path.getsize(T.DIGESTS), "bytes;", len(out), "cases")
