"""Child process of tests/test_tsdf_walk_visit_words_gpu.py (PLVS_HIP_TSDF_TRACE is read once per process): the long rays of
an oblique far wall through the 1 536-entry instance of the lean walk, whose log keeps 15 visits per ray.

Four calls of 81 images of 64 x 32 pixels (324 tiles each: long calls; in calls 2 - 4 nine are the wall and 72 hold no
valid pixel) into a 5 cm map, the lens of
test_tsdf_walk_phase_loads' wall camera twice as long so that a tile meets 400 - 540 voxels:
  1. walls at 1.0 - 3.0 m under the short lens — light tiles: the handle's first pass takes the small table from the next
     call on;
  2. the wall at 4.6 m — tiles with 10, 17 and 100 late visits behind a 15-visit log: the list;
  3. the wall at 4.8 m — every tile above the list's 128, two of them (329, 450) far above: the second walk;
  4. the wall at 4.8 m under the short lens: 1 345 - 1 792 voxels per tile, which a 2 048-entry first pass would hold and the
     small table defers — the trace of this call shows which table calls 2 and 3 ran in.
Every property is asserted from the oracle before the device runs; after every call the device map is compared with the
oracle's (tests.test_tsdf_walk_phase_loads._against_oracle) through the depth entry, and the point-stream entry's map with the
depth entry's bit for bit."""
import sys

import numpy as np

from tests import oracle_lib
from tests.test_tsdf_chisel import compare_maps
from tests.test_tsdf_chisel_depth import _clouds, _integrate_clouds, _integrate_depth
from tests.test_tsdf_walk_phase_loads import MAX_DEPTH, MIN_DEPTH, WALL_CAM, WALL_H, WALL_W, _against_oracle, _visits_per_ray, _wall_frame

LIST_CAP = 128        # FastShared::kSpillCap
SMALL_LOG = 15        # FastShared<1536>::kLogLen
SMALL_LIMIT = 1344    # entries a tile may use in the 1 536-entry table, 1 792 in the 2 048-entry one
COPIES = 81           # images per call: 324 tiles, a long call
FAR_COPIES = 9        # ... of which the far walls' calls fill with the wall


def _tile_of_pixel():
    yy, xx = np.mgrid[0:WALL_H, 0:WALL_W]
    return ((yy // 16) * (WALL_W // 32) + xx // 32).ravel()


def _voxels_per_tile(oracle, cloud):
    tile, out = _tile_of_pixel(), []
    for t in range(4):
        sel = np.flatnonzero(tile == t)
        scratch = oracle.chisel(0.05)
        scratch.integrate(cloud["xyz"][sel], cloud["rgb"][sel], cloud["kfid"][sel], cloud["Twc"])
        out.append(sum(int((scratch.get_chunk(*c)[1] > 0).sum()) for c in scratch.chunk_ids()))
    return out


def _late_per_tile(oracle, cloud):
    late, tile = np.maximum(_visits_per_ray(oracle, cloud) - SMALL_LOG, 0), _tile_of_pixel()
    return [int(late[tile == t].sum()) for t in range(4)]


def main():
    import torch
    from plvs_amd.tsdf import TsdfChisel
    oracle = oracle_lib.load()
    long_lens = oracle.cam_grid_points(WALL_W, WALL_H, 1, 2 * WALL_CAM["f"], 2 * WALL_CAM["f"], 2 * WALL_CAM["cx"], 2 * WALL_CAM["cy"])
    short_lens = oracle.cam_grid_points(WALL_W, WALL_H, 1, WALL_CAM["f"], WALL_CAM["f"], WALL_CAM["cx"], WALL_CAM["cy"])
    # (call 1: 81 walls 2.5 cm apart, so that no voxel takes tens of thousands of visits in one call — the oracle's
    # sequential float mean would drift past the tolerance the maps are compared with)
    # (calls 2 - 4: nine copies of the wall and 72 images without a valid pixel — tiles that end behind their first barrier
    # —, for the same reason: 324 tiles make the call a long one, nine visits a ray and voxel keep the float sums close)
    def padded(frame):
        empty = dict(frame, depth=np.zeros_like(frame["depth"]))
        return [frame] * FAR_COPIES + [empty] * (COPIES - FAR_COPIES)
    scenes = [([_wall_frame(1.0 + 0.025 * i, 2) for i in range(COPIES)], short_lens), (padded(_wall_frame(4.6, 1)), long_lens),
              (padded(_wall_frame(4.8, 1)), long_lens), (padded(_wall_frame(4.8, 1)), short_lens)]
    calls = []
    for k, (frames, grid) in enumerate(scenes):
        kfids = list(range(1000 * (k + 1), 1000 * (k + 1) + COPIES))
        clouds = _clouds(oracle, frames, grid, 1, MIN_DEPTH, MAX_DEPTH, kfids)
        assert all(len(c["xyz"]) in (0, WALL_W * WALL_H) for c in clouds) and len(clouds[0]["xyz"]) > 0      # (point i is pixel i)
        calls.append((frames, kfids, grid, [c for c in clouds if len(c["xyz"])]))
    # ---- what the scenes are, from the oracle (call 1: its nearest and its farthest wall)
    voxels = [_voxels_per_tile(oracle, c[3][0]) for c in calls]
    voxels[0] = [max(a, b) for a, b in zip(voxels[0], _voxels_per_tile(oracle, calls[0][3][-1]))]
    print("voxels per tile, calls 1 - 4:", voxels, flush=True)
    assert all(max(v) <= SMALL_LIMIT for v in voxels[:3])                       # nothing for the small table to defer
    assert any(SMALL_LIMIT < n <= 1792 for n in voxels[3]) and max(voxels[3]) <= 1792
    late2, late3 = _late_per_tile(oracle, calls[1][3][0]), _late_per_tile(oracle, calls[2][3][0])
    print("late visits per tile behind a 15-visit log: call 2", late2, "call 3", late3, flush=True)
    assert sum(1 <= n <= LIST_CAP for n in late2) >= 3                            # the list (10, 17, 100)
    assert min(late3) > LIST_CAP and sum(n >= 2 * LIST_CAP for n in late3) >= 2   # the second walk (329 and 450 relied on)
    # ---- the device: after every call the depth entry against the oracle, the point-stream entry against the depth entry
    ora = oracle.chisel(0.05)
    dev = TsdfChisel(0.05, max_chunks=4096, order_free=True)
    pts = TsdfChisel(0.05, max_chunks=4096, order_free=True)
    for k, (frames, kfids, grid, clouds) in enumerate(calls):
        visits = 0
        for c in clouds:
            ora.integrate(c["xyz"], c["rgb"], c["kfid"], c["Twc"])
            visits += ora.last_visits()
        _integrate_depth(dev, frames, grid, 1, MIN_DEPTH, MAX_DEPTH, kfids)      # (trace lines: depth, then points, per call)
        _integrate_clouds(pts, clouds)
        torch.cuda.synchronize()
        assert dev.last_stats()["visits"] == pts.last_stats()["visits"] == visits > 0
        assert compare_maps(dev, pts) >= 1          # the two entries: bit for bit
        n = _against_oracle(ora, dev, f"call {k + 1}")
        print(f"call {k + 1} ok chunks {n}", flush=True)
    dev.close()
    pts.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
