"""LineMatcher::FuseSearch and FuseSearchPointsAndLines of include/plvs_hip.hpp: tests/host/line_fuse_smoke.cpp compiles against
nothing but the C ABI and gives the golden candidates of tests/line_fuse_scenario.py through the host entry (no GPU), through the
device entry and through the one-wait entry."""
import os
import subprocess

import numpy as np
import pytest

from tests import line_fuse_restatement as R
from tests import line_fuse_scenario as S
from tests.test_line_fuse import GOLDEN, _write_pair_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "line_fuse_smoke.cpp")
LIB_DIR = os.path.join(ROOT, "plvs_amd", "lib")


def _run(tmp_path, where):
    exe = str(tmp_path / "line_fuse_smoke")
    subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC,
                    "-L", LIB_DIR, "-l:libplvs_hip.so", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    inp = S.inputs()
    path = str(tmp_path / "inputs.bin")
    _write_pair_input(path, inp)
    r = subprocess.run([exe, path, where], capture_output=True, text=True)
    assert r.returncode == 0 and "line_fuse_smoke ok" in r.stdout, r.stdout[-500:] + r.stderr
    g = np.load(GOLDEN)
    cand = g["reached"] == R.CANDIDATE
    want = np.stack([np.where(cand, g["raw_best_idx"], -1).reshape(-1), np.where(cand, g["raw_best_dist"], -1).reshape(-1),
                     g["reached"].reshape(-1)], 1).astype(np.int64)
    got = np.array([[int(c) for c in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("pair ")], np.int64)
    assert got.shape == want.shape and (got == want).all(), np.argwhere(got != want)[:8]
    said = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln and not ln.startswith("pair ")}
    assert said["found"][0] == str(int(cand.sum())) and said["refused"] == ["2"]
    return said, g


def test_line_fuse_cpp_mirror_on_the_host_gives_the_golden_candidates(tmp_path):
    said, g = _run(tmp_path, "host")
    assert said["found"][2:5] == ["0", str(int((g["reached"] >= R.EMPTY_WINDOW).sum())), "0"]


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["device", "both"])
def test_line_fuse_cpp_mirror_on_the_device_gives_the_golden_candidates(tmp_path, where):
    said, g = _run(tmp_path, where)
    assert said["found"][3:5] == [str(int((g["reached"] >= R.EMPTY_WINDOW).sum())), "1"]
    if where == "both":
        assert said["found"][6:] == ["1", "1"]          # the lines' launch alone (no points), one wait
