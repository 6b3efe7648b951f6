"""The bucket arithmetic of the walk's LDS voxel tables (plvs_amd/csrc/tsdf_walk_table.hpp) on a CPU: the small table of the
lean walk has 384 buckets of four keys, not a power of two — its home bucket is floor(table key * 384 / 2^32) and its probe
sequence wraps with a compare.  tests/host/walk_table_host.cpp replays table_find_or_insert key by key:

  * every table key maps into [0, 384), the buckets take equal ranges of keys, the wrap visits each bucket once;
  * realistic tile key sets up to the entry limit (7/8 of the slots: 1 344) — wall patches along each axis, oblique
    slabs, a 12 x 12 x 9 box, at five origins of the 1024^3 key box, in scan order and shuffled — all find their place
    before an insertion reaches kProbeCap (24), and are found again;
  * the same sets cut to 896 entries in 256 buckets (the table it replaced) and to 1 792 in 512 stay under the cap too.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_CAP = 24
SETS = 9 * 5   # key sets x origins per table


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    exe = tmp_path_factory.mktemp("walk_table") / "walk_table_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "host", "walk_table_host.cpp"),
                    "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    return p


def test_host_replay_passes(replay):
    assert replay.returncode == 0, replay.stdout[-2000:] + replay.stderr[-2000:]
    assert replay.stdout.strip().splitlines()[-1] == "ok"
    for buckets in (384, 256, 512):
        assert f"buckets {buckets} index functions ok" in replay.stdout


@pytest.mark.parametrize("buckets,limit", [(384, 1344), (256, 896), (512, 1792)])
def test_no_insertion_reaches_the_probe_cap(replay, buckets, limit):
    assert replay.returncode == 0, replay.stdout[-2000:]
    rows = [(int(m.group(1)), m.group(2), int(m.group(3)))
            for m in re.finditer(rf"^buckets {buckets} entries (\d+) set (\S+) at \S+ longest_search (\d+)$", replay.stdout, re.M)]
    assert len(rows) == SETS
    assert max(r[0] for r in rows) == limit, "no set at the entry limit"
    assert sum(r[0] == limit for r in rows) >= 7 * 5
    assert {r[1] for r in rows} >= {"slab_x", "slab_y", "slab_z", "oblique_123", "oblique_2m11", "oblique_5m27", "box_12x12x9"}
    worst = max(r[2] for r in rows)
    print(f"{buckets} buckets, up to {limit} entries: longest search {worst} buckets")
    assert 1 <= worst < PROBE_CAP
