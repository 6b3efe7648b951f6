"""The lean order-free walk (tsdf_walk.hpp: walk_fast_tile) where it requests its data ahead of use:

  set-up  the grid description in one burst, the pixel's depth and its (gx, gy) together — the (gx, gy) entry is read for
          every pixel of the grid, whatever its depth turns out to be, and for no other pixel;
  flush   the directory's home entry as a (key, slot) pair (dir_find_or_insert_hit), everything but a hit with a published
          slot through dir_find_or_insert.

And the ray masks it builds from the visit logs, at every log length and over more than one round of masks: the scenes a
change of that loop has to pass (one that read the log in batches of eight was measured slower and is not in the kernel).

Reference: the CPU oracle, oracle.cloudgen + oracle.chisel(...).integrate.  Against it kfid, colour, colour weight (as
tests/test_tsdf_chisel.py states it: frozen at 254) and the set of observed voxels are exact, sdf and weight within that
file's order-free tolerances (2e-5 m, 5e-5 relative).  And the depth entry and the point-stream entry of the device —
walk_fast<.., true> and walk_fast<.., false> — leave bit-identical maps (compare_maps).

What a scene must contain (rays of 14 / 15 / 16 / 17 visits, tiles of more voxels than a mask round holds, chunks beyond
their home entry, cold and saturated voxels side by side) is established on the CPU, from the oracle, before the device
runs.  The small calls run walk_fast<4096> (16-visit log, eight entries per thread); the last test goes through the
1 536-entry instance (15-visit log, three entries per thread) in a child process, as tests/test_tsdf_walk_small_table.py
does."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import oracle_lib
from tests.plvs_amd_synth import TUM1, make_rgbd_frames
from tests.test_tsdf_chisel import ORDER_FREE_COLOUR_ATOL, ORDER_FREE_SDF_ATOL, ORDER_FREE_WEIGHT_RTOL, compare_maps
from tests.test_tsdf_chisel_depth import _clouds, _integrate_clouds, _integrate_depth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_DEPTH, MAX_DEPTH = 0.1, 5.0
assert ORDER_FREE_COLOUR_ATOL == 0


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


def _against_oracle(ora, dev, what):
    """kfid, colour, colour weight, observed set exact; sdf / weight within the order-free tolerances."""
    ids = {tuple(int(v) for v in x) for x in ora.chunk_ids()}
    assert ids == {tuple(int(v) for v in x) for x in dev.chunk_ids()}, f"{what}: the sets of chunks differ"
    worst = [0.0, 0.0]
    for cid in sorted(ids):
        a, b = ora.get_chunk(*cid), dev.get_chunk(*cid)
        known = a[1] > 0
        assert np.array_equal(known, b[1] > 0), f"{what}: the sets of observed voxels of chunk {cid} differ"
        assert np.array_equal(a[2], b[2]), f"{what}: kfid of chunk {cid}"
        if not known.any():
            continue
        ca, cb = a[3][known], b[3][known]
        assert np.array_equal(np.minimum(ca >> 24, 254), np.minimum(cb >> 24, 254)), f"{what}: colour weights of chunk {cid}"
        assert np.array_equal(ca & 0xFFFFFF, cb & 0xFFFFFF), f"{what}: colours of chunk {cid}"
        worst[0] = max(worst[0], float(np.abs(a[0][known] - b[0][known]).max()))
        worst[1] = max(worst[1], float((np.abs(a[1][known] - b[1][known]) / a[1][known]).max()))
    print(f"{what}: {len(ids)} chunks, sdf {worst[0]:.3g} m, weight {worst[1]:.3g} relative")
    assert worst[0] <= ORDER_FREE_SDF_ATOL and worst[1] <= ORDER_FREE_WEIGHT_RTOL, f"{what}: {worst}"
    return len(ids)


def _both_entries(oracle, res, calls, grid, step, max_chunks, pitched=False, after_call=None):
    """Every call of `calls` ((frames, key-frame ids) each) into one oracle map, one device map through the depth entry and
    one through the point-stream entry; after every call the three are compared."""
    import torch
    from plvs_amd.tsdf import TsdfChisel
    ora = oracle.chisel(res)
    a = TsdfChisel(res, max_chunks=max_chunks, order_free=True)
    b = TsdfChisel(res, max_chunks=max_chunks, order_free=True)
    for k, (frames, kfids) in enumerate(calls):
        clouds = _clouds(oracle, frames, grid, step, MIN_DEPTH, MAX_DEPTH, kfids)
        visits = 0
        for c in clouds:
            ora.integrate(c["xyz"], c["rgb"], c["kfid"], c["Twc"])
            visits += ora.last_visits()
        if after_call is not None:
            after_call(k, ora, clouds)
        _integrate_depth(a, frames, grid, step, MIN_DEPTH, MAX_DEPTH, kfids, pitched=pitched)
        _integrate_clouds(b, clouds)
        torch.cuda.synchronize()
        assert a.last_stats()["visits"] == b.last_stats()["visits"] == visits > 0
        assert compare_maps(a, b) >= 1          # the two entries: bit for bit
        _against_oracle(ora, a, f"call {k + 1}")
    a.close()
    b.close()


def _pose(k):
    """Camera k: a few centimetres and a degree of yaw away from camera 0."""
    t = np.deg2rad(1.5 * k)
    T = np.zeros((3, 4), np.float32)
    T[:, :3] = np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]], np.float32)
    T[:, 3] = (0.03 * k, -0.02 * k, 0.01 * k)
    return T


# ------------------------------------------------------------------ 1. ragged grid, strides, invalid depths
RAGGED_W, RAGGED_H = 75, 43     # step 2: a grid of 38 x 22 = 2 x 2 tiles, the last column block 6 wide, the last band 6 high


def _ragged_frame(k):
    """A bumpy surface 1 - 2.6 m away with every kind of invalid depth in it, and by image region (tiles of the step-2 and
    of the step-1 grid alike): columns 64.. of rows ..31 hold no valid pixel; columns 64.. of rows 32.. are valid only in
    the image's last row and last column."""
    rng = np.random.default_rng(100 + k)
    w, h = RAGGED_W, RAGGED_H
    yy, xx = np.mgrid[0:h, 0:w]
    d = (1.8 + 0.6 * np.sin(xx / 9.0 + k) * np.cos(yy / 7.0) + 0.2 * rng.random((h, w))).astype(np.float32)
    bad = np.array([0.0, np.nan, -1.0, 25.0], np.float32)
    hit = rng.random((h, w)) < 0.12
    d[hit] = bad[rng.integers(0, 4, int(hit.sum()))]
    # the float nearest min_depth is inside (as a double it exceeds 0.1), max_depth itself is not, its predecessor is
    assert float(np.float32(MIN_DEPTH)) > MIN_DEPTH and float(np.float32(MAX_DEPTH)) == MAX_DEPTH
    for j, v in enumerate((np.float32(MIN_DEPTH), np.float32(MAX_DEPTH), np.nextafter(np.float32(MAX_DEPTH), np.float32(0)))):
        d[2 * j:30:6, 4 + 2 * j:60:10] = v
    d[:32, 64:] = bad[rng.integers(0, 4, (32, w - 64))]
    d[32:, 64:] = 0.0
    d[h - 1, 64:] = 1.5 + 0.05 * np.arange(w - 64, dtype=np.float32)
    d[32:, w - 1] = 2.2 - 0.04 * np.arange(h - 32, dtype=np.float32)
    valid = (d.astype(np.float64) > MIN_DEPTH) & (d.astype(np.float64) < MAX_DEPTH)
    assert not valid[:32, 64:].any() and not valid[32:h - 1, 64:w - 1].any() and valid[h - 1, 64:].all() and valid[32:, w - 1].all()
    return dict(depth=d, bgr=rng.integers(0, 256, (h, w, 3), dtype=np.uint8), Twc=_pose(k))


@pytest.mark.gpu
@pytest.mark.parametrize("step,nframes", [(2, 1), (2, 3), (1, 1), (3, 1)], ids=["step2_n1", "step2_n3", "step1", "step3"])
def test_hip_ragged_pitched_grid_with_invalid_depths(oracle, step, nframes):
    """Pitched rows and images (n = 1: the wrapper's image-stride special case); the (gx, gy) load ahead of the depth test."""
    grid = oracle.cam_grid_points(RAGGED_W, RAGGED_H, step, TUM1["fx"] / 8, TUM1["fy"] / 8, RAGGED_W / 2, RAGGED_H / 2)
    frames = [_ragged_frame(k) for k in range(nframes)]
    _both_entries(oracle, 0.05, [(frames, [40 + k for k in range(nframes)])], grid, step, 2048, pitched=True)


# ------------------------------------------------------------------ 2. mask building
WALL_W, WALL_H = 64, 32          # step 1: 2 x 2 tiles
WALL_CAM = dict(f=150.0, cx=-130.0, cy=-95.0)    # the principal point far outside the image: every ray is oblique


def _wall_frame(z, seed):
    rng = np.random.default_rng(seed)
    return dict(depth=np.full((WALL_H, WALL_W), z, np.float32), bgr=rng.integers(0, 256, (WALL_H, WALL_W, 3), dtype=np.uint8),
                Twc=np.eye(4, dtype=np.float32)[:3].copy())


def _visits_per_ray(oracle, cloud):
    """One-point clouds into a scratch map: the visits of a ray do not depend on the map."""
    scratch = oracle.chisel(0.05)
    out = np.zeros(len(cloud["xyz"]), np.int64)
    for i in range(len(out)):
        scratch.integrate(cloud["xyz"][i:i + 1], cloud["rgb"][i:i + 1], cloud["kfid"][i:i + 1], cloud["Twc"])
        out[i] = scratch.last_visits()
    return out


def _cold_voxels_per_tile(oracle, cloud):
    """Voxels a tile of 32 x 16 pixels touches in an empty map (all below colour weight 254 there)."""
    idx = np.arange(WALL_W * WALL_H).reshape(WALL_H, WALL_W)
    out = []
    for ty in range(WALL_H // 16):
        for tx in range(WALL_W // 32):
            sel = idx[16 * ty:16 * ty + 16, 32 * tx:32 * tx + 32].ravel()
            scratch = oracle.chisel(0.05)
            scratch.integrate(cloud["xyz"][sel], cloud["rgb"][sel], cloud["kfid"][sel], cloud["Twc"])
            out.append(sum(int((scratch.get_chunk(*c)[1] > 0).sum()) for c in scratch.chunk_ids()))
    return out


@pytest.mark.gpu
def test_hip_masks_from_logs_of_every_length(oracle):
    """A fronto-parallel wall at 4.8 m into an empty map: logs of at most 14, of 15, of 16 and of more than 16 visits (the
    re-walk behind a full log), more cold voxels per tile than one mask round holds; the same call once more when some
    voxels have saturated and others have not."""
    grid = oracle.cam_grid_points(WALL_W, WALL_H, 1, WALL_CAM["f"], WALL_CAM["f"], WALL_CAM["cx"], WALL_CAM["cy"])
    far = _wall_frame(4.8, 1)
    cloud = _clouds(oracle, [far], grid, 1, MIN_DEPTH, MAX_DEPTH, [7])[0]
    assert len(cloud["xyz"]) == WALL_W * WALL_H      # (so that point i is pixel i)
    v = _visits_per_ray(oracle, cloud)
    classes = [int((v <= 14).sum()), int((v == 15).sum()), int((v == 16).sum()), int((v >= 17).sum())]
    tiles = _cold_voxels_per_tile(oracle, cloud)
    print("rays with <= 14 / 15 / 16 / >= 17 visits:", classes, "cold voxels per tile:", tiles)
    assert min(classes) > 0
    # two mask rounds: more than 384 runs in the 1 536-entry instance — and more than 1 024 in the 4 096-entry one, which
    # is the one this call runs
    assert max(tiles) > 384 and max(tiles) > 1024 and max(tiles) <= 3584

    def mixed(k, ora, clouds):
        if k == 1:   # behind the 90 copies: voxels three rays of an image reach have saturated, those of one ray have not
            cw = np.concatenate([(ora.get_chunk(*c)[3] >> 24)[ora.get_chunk(*c)[1] > 0] for c in ora.chunk_ids()])
            print("colour weights behind call 2: %d voxels below 254, %d at or above" % ((cw < 254).sum(), (cw >= 254).sum()))
            assert (cw < 254).sum() > 100 and (cw >= 254).sum() > 100
    _both_entries(oracle, 0.05, [([far], [7]), ([far] * 90, list(range(100, 190))), ([far], [8])], grid, 1, 2048, after_call=mixed)


@pytest.mark.gpu
def test_hip_masks_from_short_logs(oracle):
    """The wall at 1.0 m: short logs, of lengths that are no multiple of eight."""
    grid = oracle.cam_grid_points(WALL_W, WALL_H, 1, WALL_CAM["f"], WALL_CAM["f"], WALL_CAM["cx"], WALL_CAM["cy"])
    near = _wall_frame(1.0, 2)
    v = _visits_per_ray(oracle, _clouds(oracle, [near], grid, 1, MIN_DEPTH, MAX_DEPTH, [9])[0])
    print("visits per ray:", {int(k): int((v == k).sum()) for k in np.unique(v)})
    assert v.max() < 16 and len({int(k) % 8 for k in np.unique(v)}) >= 3
    _both_entries(oracle, 0.05, [([near], [9])], grid, 1, 2048)


# ------------------------------------------------------------------ 3. directory
def _spread_frames():
    """Five cameras nine metres apart: 447 chunks of 2 cm voxels."""
    frames = make_rgbd_frames(5, seed=7, holes=True)
    for k, f in enumerate(frames):
        T = np.array(f["Twc"], np.float32).copy()
        T[0, 3] += 9.0 * k
        T[2, 3] -= 0.37 * 9.0 * k
        f["Twc"] = T
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("max_chunks", [8192, 512], ids=["roomy", "crowded"])
def test_hip_directory_inserts_then_hits(oracle, max_chunks):
    """Call 1 into a fresh map: every chunk is entered by racing threads.  Call 2, the same frames: every lookup is a hit.
    `crowded`: a pool of 512 chunks has a directory of 1 024 entries (twice the pool, the most a handle allows: it is never
    more than half full), 447 of them taken — 44 % — and, by the hash, dozens of chunks away from their home entry; the pool
    itself is not exhausted."""
    step, res = 2, 0.02
    grid = oracle.cam_grid_points(640, 480, step, TUM1["fx"], TUM1["fy"], TUM1["cx"], TUM1["cy"])
    frames = _spread_frames()

    def crowd(k, ora, clouds):
        if k == 0 and max_chunks == 512:
            ids = np.array(ora.chunk_ids(), np.int64)
            home = ((ids[:, 0] * 73856093) ^ (ids[:, 1] * 19349663) ^ (ids[:, 2] * 83492791)) & 1023    # dir_hash, 1 024 entries
            print(f"{len(ids)} chunks, {len(set(home.tolist()))} distinct home entries")
            assert 0.40 * 1024 <= len(ids) <= 512 - 32 and len(ids) - len(set(home.tolist())) >= 50
    _both_entries(oracle, res, [(frames, [60 + k for k in range(5)]), (frames, [70 + k for k in range(5)])], grid, step, max_chunks,
                  after_call=crowd)


# ------------------------------------------------------------------ 4. the hot instance: 1 536 entries, 15-visit log
def _scenario_main():
    """Child process (PLVS_HIP_TSDF_TRACE is read once per process): three calls of three 640 x 480 stride-2 images, 450
    tiles each, into a 5 cm map.  Call 1 — a frontal wall at 1.5 m, light tiles — switches the handle's first pass to the
    small table; call 2 — the wall receding from 3 m to 4.9 m of tests/walk_small_table_scenario.py, at 5 cm 250 - 800 voxels
    per tile: nothing for the small table to defer — and call 3, the same images again, run through it."""
    import torch
    from plvs_amd.tsdf import TsdfChisel
    from tests.walk_small_table_scenario import wall_frames
    oracle = oracle_lib.load()
    step, res = 2, 0.05
    grid = oracle.cam_grid_points(640, 480, step, TUM1["fx"], TUM1["fy"], TUM1["cx"], TUM1["cy"])
    oblique = wall_frames("oblique", 2)
    calls = [(wall_frames("frontal", 1), [10, 11, 12]), (oblique, [20, 21, 22]), (oblique, [30, 31, 32])]
    clouds = [_clouds(oracle, fr, grid, step, MIN_DEPTH, MAX_DEPTH, kf) for fr, kf in calls]
    # rays beyond the 15-visit log of the small table's tiles (a sample: every 37th point of call 2's first image)
    sample = {k: v[::37] if k != "Twc" else v for k, v in clouds[1][0].items()}
    v = _visits_per_ray(oracle, sample)
    print("sampled rays with <= 14 / 15 / >= 16 visits:", int((v <= 14).sum()), int((v == 15).sum()), int((v >= 16).sum()), flush=True)
    assert (v <= 14).sum() > 0 and (v == 15).sum() > 0 and (v >= 16).sum() > 0
    for entry in ("depth", "clouds"):
        ora = oracle.chisel(res)
        dev = TsdfChisel(res, max_chunks=8192, order_free=True)
        for k, ((fr, kf), cl) in enumerate(zip(calls, clouds)):
            for c in cl:
                ora.integrate(c["xyz"], c["rgb"], c["kfid"], c["Twc"])
            if entry == "depth":
                _integrate_depth(dev, fr, grid, step, MIN_DEPTH, MAX_DEPTH, kf)
            else:
                _integrate_clouds(dev, cl)
            torch.cuda.synchronize()
            n = _against_oracle(ora, dev, f"{entry} call {k + 1}")
            print(f"{entry} call {k + 1} ok chunks {n}", flush=True)
        dev.close()
    return 0


@pytest.mark.gpu
def test_hip_small_table_instance_against_the_oracle_through_both_entries():
    env = dict(os.environ, PLVS_HIP_TSDF_TRACE="1")
    p = subprocess.run([sys.executable, "-m", "tests.test_tsdf_walk_phase_loads"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    done = [ln.split()[:3] for ln in p.stdout.splitlines() if " ok chunks " in ln]
    assert done == [[e, "call", str(k)] for e in ("depth", "clouds") for k in (1, 2, 3)]
    calls = [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"\[tsdf_chisel\] tiles (\d+) deferred (\d+) split ", p.stderr)]
    print("tiles, deferred per call:", calls)
    assert len(calls) == 6 and all(c[0] == 450 for c in calls)
    # the depth entry: no tile deferred by any pass, in any call — calls 2 and 3 are the small table's from end to end
    assert [c[1] for c in calls[:3]] == [0, 0, 0]


if __name__ == "__main__":
    sys.exit(_scenario_main())
