"""BowSearch of include/plvs_hip.hpp: tests/host/bow_search_smoke.cpp compiles against nothing but the C ABI, flattens std::map feature
vectors as the mirror does and must give what the host twin gives through the Python mirror (no GPU), and the same through the device entries."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import bow_search_restatement as R
from tests import bow_search_scenario as S
from tests.test_bow_search import Handles, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "bow_search_smoke.cpp")
LIB_DIR = os.path.join(ROOT, "plvs_amd", "lib")
RATIO, ORI = 0.9, 1


def _write(path, a_side, b_sides):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<i", len(b_sides)))
        for s in [a_side] + list(b_sides):
            fh.write(struct.pack("<ii", len(s["desc"]), len(s["nodes"])))
            fh.write(np.ascontiguousarray(s["desc"], np.uint8).tobytes() + np.ascontiguousarray(s["angle"], np.float32).tobytes() + S.valid_of(s).tobytes())
            for node, lst in sorted(s["nodes"].items()):
                fh.write(struct.pack("<Ii", node, len(lst)) + np.array(lst, np.uint32).tobytes())


def _run(tmp_path, where):
    exe = str(tmp_path / "bow_search_smoke")
    subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC,
                    "-L", LIB_DIR, "-l:libplvs_hip.so", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    a_side, b_sides = S.calls()["main"]
    path = str(tmp_path / "inputs.bin")
    _write(path, a_side, b_sides)
    r = subprocess.run([exe, path, where, str(RATIO), str(ORI)], capture_output=True, text=True)
    assert r.returncode == 0 and "bow_search_smoke ok" in r.stdout and "refused 1" in r.stdout, r.stdout[-500:] + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    lens = [len(v) for v in a_side["nodes"].values()]
    assert [ln[1:] for ln in lines if ln[0] == "bow_info"] == [[str(len(lens)), str(sum(lens)), str(max(lens))]]
    stats = {}
    with Handles(a_side, b_sides, host_only=True) as h:
        for kind in (R.KF, R.FRAME):
            match, dist, n, st = search(h, kind, RATIO, ORI, True)        # the host twin
            got_n = [[int(c) for c in ln[2:]] for ln in lines if ln[:2] == [kind, "nmatches"]]
            assert got_n == [n.tolist()]
            got = sorted((int(ln[2]), int(ln[3]), int(ln[4])) for ln in lines if ln[:2] == [kind, "match"])
            flat_m, flat_d = match.reshape(-1), dist.reshape(-1)
            assert got == [(int(i), int(flat_m[i]), int(flat_d[i])) for i in np.flatnonzero(flat_m >= 0)] and len(got) == int(n.sum()) > 20
            (head,) = [ln for ln in lines if ln[:2] == [kind, "total"]]
            assert int(head[2]) == int(n.sum())
            stats[kind] = ([int(c) for c in head[4:]], st.tolist())
    return stats


def test_bow_search_cpp_mirror_on_the_host_equals_the_host_twin(tmp_path):
    for said, twin in _run(tmp_path, "host").values():
        assert said == twin and said[:3] == [0, 0, 0]


@pytest.mark.gpu
def test_bow_search_cpp_mirror_on_the_device_equals_the_host_twin(tmp_path):
    for said, twin in _run(tmp_path, "device").values():
        assert said[0] == 1 and said[1] == 1 and said[2] > 0 and said[3:] == twin[3:]
