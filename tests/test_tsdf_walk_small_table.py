"""The small table of the lean order-free walk (tsdf_walk.hpp: walk_fast<kFastEntriesSmall> = 1 536 entries in 384 buckets,
not a power of two) on the device, on tiles around its entry limit.

tests/walk_small_table_scenario.py (3.5 cm voxels): call 1 (a frontal wall at 1.5 m, light tiles) switches the handle's
first pass to the small table; call 2 (a wall receding from 3 to 4.9 m, 510 - 2 000 voxels per tile) fills it: tiles beyond
its 1 344 entries are deferred to the 2 048-entry pass, the others are walked once.  After each call the map equals the
oracle's sequential integrate — kfid, colour and the set of observed voxels exactly, sdf within 2e-5 m, weight within 5e-5
relative — through the depth entry (walk_fast<.., true>) and through the point-stream entry (walk_fast<.., false>).

The trace line of a call carries `deferred` = 1000 x (tiles the first lean pass deferred) + (tiles the second deferred)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = 450


@pytest.fixture(scope="module")
def scenario():
    env = dict(os.environ, PLVS_HIP_TSDF_TRACE="1")
    p = subprocess.run([sys.executable, "-m", "tests.walk_small_table_scenario"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    calls = [(int(m.group(1)), int(m.group(2)), int(m.group(3)))
             for m in re.finditer(r"\[tsdf_chisel\] tiles (\d+) deferred (\d+) split (\d+) ", p.stderr)]
    for ln in p.stdout.strip().splitlines():
        print(ln)
    for c in calls:
        print("tiles %d deferred: first pass %d, second pass %d, third %d; split %d" % (c[0], c[1] // 1000 % 1000, c[1] % 1000, c[1] // 1000000, c[2]))
    return p, calls


@pytest.mark.gpu
def test_hip_maps_equal_the_oracle_through_both_entries(scenario):
    p, calls = scenario
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    lines = [ln.split() for ln in p.stdout.strip().splitlines()]
    assert [(ln[0], ln[2]) for ln in lines] == [("depth", "1"), ("depth", "2"), ("clouds", "1"), ("clouds", "2")]
    assert all(int(ln[4]) > 0 for ln in lines)
    assert len(calls) == 4 and all(c[0] == TILES for c in calls)


@pytest.mark.gpu
def test_hip_small_table_defers_some_tiles_of_the_receding_wall_but_not_all(scenario):
    p, calls = scenario
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    first_call, second_call = calls[0], calls[1]     # (the depth entry's)
    # call 1: no tile beyond any lean table — and none beyond the small one, so that call 2 starts with it
    assert first_call[1] == 0 and first_call[2] == 0
    # call 2: some tiles beyond the small table, not all
    nd1, nd2, nd3 = second_call[1] // 1000 % 1000, second_call[1] % 1000, second_call[1] // 1000000
    assert 0 < nd1 < TILES, "the first pass of call 2 must defer some tiles and walk the others"
    # ... and it WAS the small table's pass: the pass behind it deferred tiles too (the tenth beyond 1 792 entries), fewer
    # than it was given.  Behind a 2 048-entry first pass stands the 4 096-entry table, which holds every tile of this wall
    # (2 000 voxels at the most against 3 584): its count would be 0.
    assert 0 < nd2 < nd1 and nd3 == 0
    # the point-stream entry took the same route: every strip of call 2 overflowed the small table
    assert calls[2][1] == 0 and calls[3][1] // 1000 % 1000 > 0
