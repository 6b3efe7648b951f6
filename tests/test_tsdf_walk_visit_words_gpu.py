"""The depth-image lean walk's two visit words, its list of late visits and its partial mask clear on the device
(plvs_amd/csrc/tsdf_walk.hpp: walk_lean<.., kVisitWords>, FastShared::spill, the mask rounds of walk_fast_tile).

Every scene's defining property is asserted on the CPU, from the oracle, before the device runs; every device map is
compared with the oracle's sequential integrate (kfid, colour, colour weight and the observed set exact, sdf and weight within
the order-free tolerances) and, depth entry against point-stream entry, bit for bit (_both_entries).

  1. a fronto-parallel wall 0.3 m away under a long lens: all 512 rays of a tile visit the same voxels — the count field of
     the count word at its maximum, the ray sum at 130 816;
  2. the oblique wall of test_tsdf_walk_phase_loads at 4.6 m and at 4.8 m, small calls (the 16-visit log of
     walk_fast<4096>): at 4.6 m one tile has 2 late visits (the list), at 4.8 m two tiles have 8 and 116 (the list) and two
     have 129 and 151, more than the list's 128 (the second walk of the long rays behind the rounds);
  3. the 4.8 m wall with one tile reduced to five valid pixels: a tile of more runs than one mask round of walk_fast<4096>
     holds (1 024; its last round clears a part of the area) beside a tile of a handful of runs;
  4. a wall at 1 m as 8 isolated pixels see it, saturated by 270 frames (a voxel takes one or two visits a frame: the
     sequential float mean of the oracle stays within the tolerance), then the same pixels at 1.10 m: their rays pass
     saturated voxels and reach new ones, and every voxel still below colour weight 254 that a tile meets has exactly ONE
     ray of the tile (the one-ray shortcut: the ray comes from the ray sum of the count word); then the pixels at 1.20 m
     with one more beside another: some such voxels have TWO rays beside the others (the masks come from the logs);
  5. tests/walk_visit_words_scenario.py in a child process: the long rays through the 1 536-entry instance and its
     15-visit log — a call whose tiles have 10, 17 and 100 late visits (the list) and a call whose tiles have 137 to 450
     (the second walk) —, the instance proven by a last call whose heavier tiles only the small table defers.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import oracle_lib
from tests.test_tsdf_chisel_depth import _clouds
from tests.test_tsdf_walk_phase_loads import (MAX_DEPTH, MIN_DEPTH, WALL_CAM, WALL_H, WALL_W, _both_entries, _visits_per_ray,
                                              _wall_frame)

LIST_CAP = 128      # FastShared::kSpillCap
LOG_LEN = 16        # visits per ray in the log of walk_fast<4096>, the instance of a small call
ROUND_RUNS = 1024   # masks per round of walk_fast<4096>


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


def _tiles_of_pixels():
    """Tile (of 32 x 16 pixels, raster order of tiles) of every pixel of the WALL_W x WALL_H image."""
    yy, xx = np.mgrid[0:WALL_H, 0:WALL_W]
    return ((yy // 16) * (WALL_W // 32) + xx // 32).ravel()


def _weights(oracle, cloud, sel):
    scratch = oracle.chisel(0.05)
    scratch.integrate(cloud["xyz"][sel], cloud["rgb"][sel], cloud["kfid"][sel], cloud["Twc"])
    w = np.concatenate([scratch.get_chunk(*c)[1].ravel() for c in scratch.chunk_ids()])
    return w[w > 0]


@pytest.mark.gpu
def test_hip_every_ray_of_a_tile_in_one_voxel(oracle):
    grid = oracle.cam_grid_points(WALL_W, WALL_H, 1, 600.0, 600.0, 31.5, 15.5)
    near = _wall_frame(0.3, 3)
    cloud = _clouds(oracle, [near], grid, 1, MIN_DEPTH, MAX_DEPTH, [5])[0]
    assert len(cloud["xyz"]) == WALL_W * WALL_H      # (so that point i is pixel i)
    tile = _tiles_of_pixels()
    one = float(_weights(oracle, cloud, np.array([0])).max())     # what one visit adds to a voxel's weight
    most = [float(_weights(oracle, cloud, np.flatnonzero(tile == t)).max()) / one for t in range(4)]
    print("most visits of a voxel, per tile:", most)
    assert max(abs(m - 512.0) for m in most) < 0.01               # a voxel all 512 rays of the tile visit, in every tile
    _both_entries(oracle, 0.05, [([near], [5]), ([near], [6])], grid, 1, 2048)


def _late_per_tile(oracle, frame, log_len):
    grid = oracle.cam_grid_points(WALL_W, WALL_H, 1, WALL_CAM["f"], WALL_CAM["f"], WALL_CAM["cx"], WALL_CAM["cy"])
    cloud = _clouds(oracle, [frame], grid, 1, MIN_DEPTH, MAX_DEPTH, [7])[0]
    assert len(cloud["xyz"]) == WALL_W * WALL_H
    late = np.maximum(_visits_per_ray(oracle, cloud) - log_len, 0)
    tile = _tiles_of_pixels()
    return grid, [int(late[tile == t].sum()) for t in range(4)]


@pytest.mark.gpu
@pytest.mark.parametrize("z,want", [(4.6, "list"), (4.8, "list_and_second_walk")], ids=["wall_4m6", "wall_4m8"])
def test_hip_late_visits_from_the_list_and_from_the_second_walk(oracle, z, want):
    frame = _wall_frame(z, 1)
    grid, late = _late_per_tile(oracle, frame, LOG_LEN)
    print("late visits per tile behind a 16-visit log:", late)
    if want == "list":
        assert max(late) >= 1 and max(late) <= LIST_CAP
    else:
        # (8 and 116 for the list; 151 is the tile relied on for the second walk, 129 lies just above the capacity)
        assert any(1 <= n <= LIST_CAP for n in late) and any(n >= LIST_CAP + 20 for n in late)
    # an empty map (every voxel below colour weight 254: masks from the logs), then the same image again
    _both_entries(oracle, 0.05, [([frame], [7]), ([frame], [8])], grid, 1, 2048)


@pytest.mark.gpu
def test_hip_partial_mask_clear_beside_a_tile_of_few_runs(oracle):
    frame = _wall_frame(4.8, 1)
    keep = [(1, 3), (4, 30), (9, 17), (12, 0), (15, 31)]         # the valid pixels of tile 0
    d = frame["depth"]
    hole = np.zeros_like(d, dtype=bool)
    hole[:16, :32] = True
    for y, x in keep:
        hole[y, x] = False
    d[hole] = 0.0
    grid = oracle.cam_grid_points(WALL_W, WALL_H, 1, WALL_CAM["f"], WALL_CAM["f"], WALL_CAM["cx"], WALL_CAM["cy"])
    cloud = _clouds(oracle, [frame], grid, 1, MIN_DEPTH, MAX_DEPTH, [7])[0]
    tile = _tiles_of_pixels()[~hole.ravel()]                     # (the cloud holds the valid pixels in raster order)
    assert len(cloud["xyz"]) == len(tile) == WALL_W * WALL_H - 512 + len(keep)
    cold = [int(len(_weights(oracle, cloud, np.flatnonzero(tile == t)))) for t in range(4)]
    print("cold voxels (runs) per tile in an empty map:", cold)
    assert cold[0] <= 18 * len(keep) and max(cold) > ROUND_RUNS and max(cold) % ROUND_RUNS != 0 and max(cold) <= 3584
    _both_entries(oracle, 0.05, [([frame], [7]), ([frame], [8])], grid, 1, 2048)


# ------------------------------------------------------------------ 4. one ray / two rays per cold voxel of a saturated map
def _voxels(chisel):
    """{(chunk id, voxel index): colour weight} of the observed voxels of an oracle map."""
    out = {}
    for c in chisel.chunk_ids():
        ch = chisel.get_chunk(*c)
        w, cw = ch[1].ravel(), ch[3].ravel() >> 24
        for i in np.flatnonzero(w > 0):
            out[(tuple(int(v) for v in c), int(i))] = int(cw[i])
    return out


def _sparse_frame(z, pixels, seed):
    frame = _wall_frame(z, seed)
    d = np.zeros_like(frame["depth"])
    for y, x in pixels:
        d[y, x] = z
    frame["depth"] = d
    return frame


def _rays_per_cold_voxel(oracle, before, frame, pixels, grid):
    """{(tile, voxel): rays of the tile that visit it} over the voxels below colour weight 254 in the map `before`."""
    cloud = _clouds(oracle, [frame], grid, 1, MIN_DEPTH, MAX_DEPTH, [1])[0]
    assert len(cloud["xyz"]) == len(pixels)          # (raster order: point i is pixels[i])
    assert pixels == sorted(pixels)
    state = _voxels(before)
    out = {}
    for i, (y, x) in enumerate(pixels):
        scratch = oracle.chisel(0.05)
        scratch.integrate(cloud["xyz"][i:i + 1], cloud["rgb"][i:i + 1], cloud["kfid"][i:i + 1], cloud["Twc"])
        for v in _voxels(scratch):
            if state.get(v, 0) < 254:
                key = ((y // 16) * (WALL_W // 32) + x // 32, v)
                out[key] = out.get(key, 0) + 1
    return out


@pytest.mark.gpu
def test_hip_one_ray_and_two_rays_per_cold_voxel_of_a_saturated_map(oracle):
    grid = oracle.cam_grid_points(WALL_W, WALL_H, 1, WALL_CAM["f"], WALL_CAM["f"], WALL_CAM["cx"], WALL_CAM["cy"])
    isolated = sorted((y, x) for y in range(2, WALL_H, 16) for x in range(3, WALL_W, 16))     # two a tile
    wall = _sparse_frame(1.0, isolated, 2)       # the wall as these pixels see it: a voxel takes one or two visits a frame
    one = _sparse_frame(1.10, isolated, 5)       # through the saturated voxels to new ones behind them
    paired = sorted(isolated + [(2, 4)])
    two = _sparse_frame(1.20, paired, 6)
    # the CPU's view, call by call
    before = oracle.chisel(0.05)
    cloud = _clouds(oracle, [wall], grid, 1, MIN_DEPTH, MAX_DEPTH, [9])[0]
    for _ in range(270):
        before.integrate(cloud["xyz"], cloud["rgb"], cloud["kfid"], cloud["Twc"])
    hot = {v for v, cw in _voxels(before).items() if cw >= 254}
    assert len(hot) > 50 and len(hot) == len(_voxels(before))        # the wall has saturated, every voxel of it
    c1 = _clouds(oracle, [one], grid, 1, MIN_DEPTH, MAX_DEPTH, [400])[0]
    scratch = oracle.chisel(0.05)
    scratch.integrate(c1["xyz"], c1["rgb"], c1["kfid"], c1["Twc"])
    met = set(_voxels(scratch))
    n1 = _rays_per_cold_voxel(oracle, before, one, isolated, grid)
    print("isolated pixels: %d saturated voxels met, %d cold (tile, voxel) pairs, rays per pair at most %d"
          % (len(met & hot), len(n1), max(n1.values())))
    assert len(met & hot) > 20                                         # tiles of a saturated map ...
    assert len(n1) > 40 and set(n1.values()) == {1} and {t for t, _ in n1} == {0, 1, 2, 3}   # ... whose cold voxels have one ray each
    before.integrate(c1["xyz"], c1["rgb"], c1["kfid"], c1["Twc"])
    n2 = _rays_per_cold_voxel(oracle, before, two, paired, grid)
    twice = [k for k, n in n2.items() if n == 2]
    print("one pixel beside another: %d cold pairs, %d of them with two rays (tiles %s)" % (len(n2), len(twice), sorted({t for t, _ in twice})))
    assert max(n2.values()) == 2 and 1 <= len(twice) and {t for t, _ in twice} == {0}
    assert sum(1 for (t, _), n in n2.items() if t == 0 and n == 1) > 10      # ... beside the others of that tile
    assert all(n == 1 for (t, _), n in n2.items() if t != 0)                 # the other tiles still take the shortcut
    calls = [([wall] * 90, list(range(100 + 90 * k, 190 + 90 * k))) for k in range(3)] + [([one], [400]), ([two], [401])]
    _both_entries(oracle, 0.05, calls, grid, 1, 2048)


# ------------------------------------------------------------------ 5. the long rays through the 1 536-entry instance
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_hip_late_visits_through_the_small_table_instance():
    env = dict(os.environ, PLVS_HIP_TSDF_TRACE="1")
    p = subprocess.run([sys.executable, "-m", "tests.walk_visit_words_scenario"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2500:] + p.stderr[-1500:]
    done = [ln.split()[:2] for ln in p.stdout.splitlines() if " ok chunks " in ln]
    assert done == [["call", str(k)] for k in (1, 2, 3, 4)]
    calls = [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"\[tsdf_chisel\] tiles (\d+) deferred (\d+) split ", p.stderr)]
    print("tiles, deferred per call (depth entry, point-stream entry, in turn):", calls)
    assert len(calls) == 8 and all(c[0] == 324 for c in calls[0::2])
    depth = calls[0::2]
    # the depth entry: calls 1 - 3 defer nothing — calls 2 and 3 are walked by their first pass from end to end —, and
    # that pass has the small table: call 4's tiles of 1 345 - 1 792 voxels would fit a 2 048-entry first pass and are deferred
    assert [c[1] for c in depth[:3]] == [0, 0, 0]
    assert depth[3][1] // 1000 % 1000 > 0
