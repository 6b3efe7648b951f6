"""The two LDS words a visit adds to in the depth-image instances of the lean walk (plvs_amd/csrc/tsdf_walk_visit.hpp) on a
CPU.  tests/host/walk_visit_host.cpp replays the packing with plain 64- and 32-bit adds, as the LDS atomics do them:

  * every single ray 0 .. 511 unpacks to (count 1, ray sum = the ray) — what the one-ray shortcut of the flush reads;
  * all 512 rays together unpack to (512, 130 816), with the largest weight a tile may carry and w * u at both ends of int32;
  * 2 000 seeded random subsets in random order, w * u at INT32_MAX / INT32_MIN / -1 / 0 / random, weights at the bound that
    keeps their sum below 2^31, match sums kept separately — so neither half of the 64-bit word carries into the other.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    exe = tmp_path_factory.mktemp("walk_visit") / "walk_visit_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "host", "walk_visit_host.cpp"),
                    "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)


def test_host_replay_passes(replay):
    assert replay.returncode == 0, replay.stdout[-2000:] + replay.stderr[-2000:]
    assert "FAILED" not in replay.stdout
    assert replay.stdout.strip().splitlines()[-1] == "ok"


def test_every_case_ran(replay):
    assert replay.returncode == 0, replay.stdout[-2000:]
    assert "single rays ok" in replay.stdout
    assert "all rays ok: count 512 ray sum 130816" in replay.stdout
    assert "random subsets ok: 2000" in replay.stdout
