"""LoopSearchByProjection of include/plvs_hip.hpp: tests/host/loop_search_smoke.cpp compiles against nothing but the C ABI and gives the
golden matches of tests/loop_search_scenario.py through the host entry (no GPU) and through the device entry."""
import os
import subprocess

import numpy as np
import pytest

from tests import loop_search_scenario as S
from tests import orb_fuse_restatement as R
from tests.test_loop_search import GOLDEN
from tests.test_orb_fuse import _write_pair_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "loop_search_smoke.cpp")
LIB_DIR = os.path.join(ROOT, "plvs_amd", "lib")
RUN = "point_camera_r15_"          # what the program asks for: PLVS_LOOP_PROJECT_CAMERA, ratio 1.5


def _run(tmp_path, where):
    exe = str(tmp_path / "loop_search_smoke")
    subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC,
                    "-L", LIB_DIR, "-l:libplvs_hip.so", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    inp = S.point_inputs()
    path = str(tmp_path / "inputs.bin")
    _write_pair_input(path, inp)          # (its Ow is the point side's: Ow_points)
    (marked,) = np.flatnonzero(inp["occupied"][0])
    assert inp["occupied"][1] is None and not inp["occupied"][2].any()
    r = subprocess.run([exe, path, where, str(int(marked))], capture_output=True, text=True)
    assert r.returncode == 0 and "loop_search_smoke ok" in r.stdout, r.stdout[-500:] + r.stderr
    g = np.load(GOLDEN)
    match = g[RUN + "match_idx"]
    want = np.stack([match.reshape(-1), np.where(match >= 0, g[RUN + "raw_best_dist"], -1).reshape(-1), g[RUN + "reached"].reshape(-1)], 1).astype(np.int64)
    got = np.array([[int(c) for c in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("pair ")], np.int64)
    assert got.shape == want.shape and (got == want).all(), np.argwhere(got != want)[:8]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln and not ln.startswith("pair ")]
    said = {ln[0]: ln[1:] for ln in lines if ln[0] != "nmatches"}
    assert [int(ln[2]) for ln in lines if ln[0] == "nmatches"] == g[RUN + "nmatches"].tolist()
    M = match.shape[1]
    assert said["found"][0] == str(int((match >= 0).sum())) and said["refused"] == ["5"] and said["twice"] == [str(M), "of", str(M)]
    return said, g


def test_loop_search_cpp_mirror_on_the_host_gives_the_golden_matches(tmp_path):
    said, g = _run(tmp_path, "host")
    assert said["found"][2:] == ["0", str(int((g[RUN + "reached"] >= R.EMPTY_WINDOW).sum())), "0", "0", "0"]


@pytest.mark.gpu
def test_loop_search_cpp_mirror_on_the_device_gives_the_golden_matches(tmp_path):
    said, g = _run(tmp_path, "device")
    assert said["found"][3:5] == [str(int((g[RUN + "reached"] >= R.EMPTY_WINDOW).sum())), "1"] and int(said["found"][5]) > 0
