"""The lean order-free walk (tsdf_walk.hpp: walk_lean / walk_fast_tile) where a voxel's LAST VISITOR decides something:
the ray index the voxel loop leaves in e_last (walk_fast takes it from the bits of the visit-log offset it carries, not
from a register of its own) names the key frame of the voxel and, for a cold voxel with one visiting ray, the one bit of
its ray mask; and the two forms of walk_fast — workgroup b walks tile b / the workgroups take the tiles of a list — are
two kernels.

Inputs: synthetic walls seen by a pinhole camera of 64 x 32 pixels at step 2 — ONE 32 x 16 tile of grid pixels per image —
or 128 x 32 (two column blocks), 5 cm voxels, through the depth entry (integrate_depth_batch_dev) as
tests/test_tsdf_chisel_depth.py drives it.

Bar of every case: against the oracle's sequential integrate of the clouds its generator makes from the same images — the
same chunks, the same observed voxels, kfid and colour exact, sdf / weight within the order-free tolerances of
tests/test_tsdf_chisel.py — and BIT-IDENTICAL to the map the point-stream entry (integrate_batch_dev) builds from those
clouds.  Cases 1-3 also against the ordered mode on the same input (observed set, kfid, colour equal).

What the cases rely on — ray lengths, rays that share no voxel, voxels per tile — is computed with the oracle on the CPU
(test_inputs_are_what_the_cases_rely_on, no GPU)."""
import functools

import numpy as np
import pytest

from tests import oracle_lib
from tests.test_tsdf_chisel import ORDER_FREE_SDF_ATOL, ORDER_FREE_WEIGHT_RTOL, compare_maps
from tests.test_tsdf_chisel_depth import _clouds, _integrate_clouds, _integrate_depth

RES = 0.05
STEP = 2
MIN_DEPTH = 0.1
H = 32
FOCAL = 600.0            # pixels: a 64 x 32 image spans 6 x 3 degrees, a tile of near rays a few hundred voxels
LOG_LEN = 16             # visits per ray the tile's log keeps (kLogLen; the 1536-entry table keeps 15)
SMALL_TABLE_LIMIT = 1536 * 7 // 8    # voxels of a tile the 1536-entry table takes (kLimit of walk_fast<1536>)
MID_TABLE_LIMIT = 2048 * 7 // 8      # ... and the 2048-entry table
LONG_CALL_TILES = 336    # > kSmallCallTiles (320, tsdf_walk_plan.hpp): the call's first pass is the 2048- or the 1536-entry table


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


def _grid(oracle, width):
    return oracle.cam_grid_points(width, H, STEP, FOCAL, FOCAL, (width - 1) / 2.0, (H - 1) / 2.0)


def _pose(x=0.0, y=0.0, z=0.0):
    Twc = np.eye(4, dtype=np.float32)[:3].copy()
    Twc[:, 3] = (x, y, z)
    return Twc


def _wall(width, dist, yaw_deg, seed, Twc=None, keep=None):
    """A plane through (0, 0, dist) of the camera frame, turned by yaw about the vertical: depth (z) per pixel, random colours.
    keep: mask of pixels that stay valid (the others: 0 = no return)."""
    u, v = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(H, dtype=np.float64))
    gx = (u - (width - 1) / 2.0) / FOCAL
    s, c = np.sin(np.radians(yaw_deg)), np.cos(np.radians(yaw_deg))
    depth = (dist * c / (gx * s + c)).astype(np.float32)
    if keep is not None:
        depth = np.where(keep, depth, np.float32(0.0)).astype(np.float32)
    bgr = np.random.default_rng(seed).integers(0, 256, (H, width, 3), dtype=np.uint8)
    return dict(depth=depth, bgr=bgr, Twc=_pose() if Twc is None else Twc)


def _sparse_mask(width):
    """every 8th grid pixel of every 8th grid row (grid pixel (m, n) = image pixel (m step, n step))"""
    keep = np.zeros((H, width), bool)
    keep[::8 * STEP, ::8 * STEP] = True
    return keep


# ---------------------------------------------------------------- the scenes (built once per process)
@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict(width, max_depth, calls=[(frames, kfids), ...])"""
    if name in ("last_visitor_one_call", "last_visitor_two_calls"):
        # two images of the same wall from the same pose: the same rays, the same voxels — other colours, other key frames
        w = 128
        a, b = _wall(w, 1.5, 25.0, seed=1), _wall(w, 1.5, 25.0, seed=2)
        pairs = [([a, b], [9, 3]), ([a, b], [3, 9])]
        if name == "last_visitor_two_calls":
            pairs = [([f], [k]) for fr, kf in pairs for f, k in zip(fr, kf)]
        return dict(width=w, max_depth=5.0, calls=pairs)
    if name == "one_ray_per_voxel":
        return dict(width=64, max_depth=5.0, calls=[([_wall(64, 3.0, 20.0, seed=3, keep=_sparse_mask(64))], [4])])
    if name == "all_pixels":
        return dict(width=64, max_depth=5.0, calls=[([_wall(64, 3.0, 20.0, seed=3)], [4])])
    if name == "long_rays_7m":
        return dict(width=64, max_depth=8.0, calls=[([_wall(64, 7.0, 40.0, seed=5), _wall(64, 7.0, 40.0, seed=6, Twc=_pose(x=0.02))], [7, 2])])
    if name == "short_rays_2m":
        return dict(width=64, max_depth=8.0, calls=[([_wall(64, 2.0, 40.0, seed=5), _wall(64, 2.0, 40.0, seed=6, Twc=_pose(x=0.02))], [7, 2])])
    if name == "tile_beyond_the_small_table":
        # two long calls (one tile per image): the first, of near walls, leaves the handle with the small table for the next
        # call's first pass; in the second every 24th image sees the far wall, whose tile the small table does not hold
        w = 64
        near = [_wall(w, 1.2 + 0.002 * (k % 50), 10.0, seed=100 + k, Twc=_pose(x=0.4 * (k % 12), y=0.3 * (k // 12 % 4)))
                for k in range(LONG_CALL_TILES)]
        mixed = [(_wall(w, 6.0, 0.0, seed=500 + k, Twc=_pose(x=0.4 * (k % 12), y=0.3 * (k // 12 % 4), z=-2.0)) if k % 24 == 5 else
                  _wall(w, 1.25 + 0.002 * (k % 50), 10.0, seed=500 + k, Twc=_pose(x=0.4 * (k % 12), y=0.3 * (k // 12 % 4))))
                 for k in range(LONG_CALL_TILES)]
        # (key frames in falling, then rising order: the largest id is not the last visitor)
        kf1 = [1000 - k for k in range(LONG_CALL_TILES)]
        kf2 = [k if k % 2 else 2000 - k for k in range(LONG_CALL_TILES)]
        return dict(width=w, max_depth=8.0, calls=[(near, kf1), (mixed, kf2)])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The oracle's map after every call of the scene (computed once, shared, never changed): [(clouds, {chunk id: arrays})]"""
    oracle = oracle_lib.load()
    sc = scene(name)
    grid = _grid(oracle, sc["width"])
    ora = oracle.chisel(RES)
    out = []
    for frames, kfids in sc["calls"]:
        clouds = _clouds(oracle, frames, grid, STEP, MIN_DEPTH, sc["max_depth"], kfids)
        for c in clouds:
            ora.integrate(c["xyz"], c["rgb"], c["kfid"], c["Twc"])
        out.append((clouds, {tuple(cid): tuple(a.copy() for a in ora.get_chunk(*cid)) for cid in ora.chunk_ids()}))
    ora.close()
    return out


def _ray_visits(oracle, cloud):
    """visits of every ray of a cloud, each integrated alone into a fresh map"""
    n = []
    for i in range(cloud["xyz"].shape[0]):
        o = oracle.chisel(RES)
        o.integrate(cloud["xyz"][i:i + 1], cloud["rgb"][i:i + 1], cloud["kfid"][i:i + 1], cloud["Twc"])
        n.append(o.last_visits())
        o.close()
    return np.array(n)


def _voxels_of(oracle, cloud):
    """(voxels, visits) of one cloud integrated into a fresh map"""
    o = oracle.chisel(RES)
    o.integrate(cloud["xyz"], cloud["rgb"], cloud["kfid"], cloud["Twc"])
    nvox = sum(int((o.get_chunk(*cid)[1] > 0).sum()) for cid in o.chunk_ids())
    visits = o.last_visits()
    o.close()
    return nvox, visits


def test_inputs_are_what_the_cases_rely_on(oracle):
    # case 1: the two images of a pair visit the same voxels
    clouds = _reference("last_visitor_one_call")[0][0]
    assert np.array_equal(clouds[0]["xyz"], clouds[1]["xyz"]) and clouds[0]["xyz"].shape[0] == 64 * 16
    # case 2: no two rays share a voxel / with every pixel valid they do
    sparse = _reference("one_ray_per_voxel")[0][0][0]
    nvox, visits = _voxels_of(oracle, sparse)
    assert sparse["xyz"].shape[0] == 2 * 4 and nvox == visits > 0
    nvox, visits = _voxels_of(oracle, _reference("all_pixels")[0][0][0])
    assert visits > nvox > 0
    # case 3: rays longer than the visit log at 7 m, none at 2 m
    far = _ray_visits(oracle, _reference("long_rays_7m")[0][0][0])
    near = _ray_visits(oracle, _reference("short_rays_2m")[0][0][0])
    print("visits per ray: 7 m wall %d..%d, 2 m wall %d..%d" % (far.min(), far.max(), near.min(), near.max()))
    assert (far > LOG_LEN).sum() >= far.size // 2 and 0 < near.max() < LOG_LEN - 1
    for c in _reference("long_rays_7m")[0][0]:
        nvox, _ = _voxels_of(oracle, c)
        print("7 m wall: %d voxels in the tile" % nvox)
        assert nvox <= 4096 * 7 // 8     # (a tile of a call of two stands in the 4096-entry table: walk_fast's own re-walk)
    # case 4: near tiles fit the small table, the far wall's do not — and fit the next one
    first, second = (r[0] for r in _reference("tile_beyond_the_small_table"))
    assert len(second) == LONG_CALL_TILES > 320
    for k in [0, 7] + list(range(5, LONG_CALL_TILES, 24)):
        nvox, _ = _voxels_of(oracle, second[k])
        print("tile %d: %d voxels" % (k, nvox))
        if k % 24 == 5:
            assert SMALL_TABLE_LIMIT < nvox <= MID_TABLE_LIMIT
        else:
            assert 0 < nvox <= SMALL_TABLE_LIMIT
    assert max(_voxels_of(oracle, c)[0] for c in first[::16]) <= SMALL_TABLE_LIMIT


def _against_reference(dev, ref_map):
    ids = {tuple(x) for x in dev.chunk_ids()}
    assert ids == set(ref_map), "the sets of chunks differ"
    worst = [0.0, 0.0]
    for cid in sorted(ids):
        a, b = ref_map[cid], dev.get_chunk(*cid)
        known = a[1] > 0
        assert np.array_equal(known, b[1] > 0), f"the sets of observed voxels of chunk {cid} differ"
        assert np.array_equal(a[2], b[2]), f"kfid of chunk {cid}"
        if not known.any():
            continue
        ca, cb = a[3][known], b[3][known]
        assert np.array_equal(np.minimum(ca >> 24, 254), np.minimum(cb >> 24, 254)), f"colour weights of chunk {cid}"
        assert np.array_equal(ca & 0xFFFFFF, cb & 0xFFFFFF), f"colours of chunk {cid}"
        worst[0] = max(worst[0], float(np.abs(a[0][known] - b[0][known]).max()))
        worst[1] = max(worst[1], float((np.abs(a[1][known] - b[1][known]) / a[1][known]).max()))
    print("sdf %.3g m, weight %.3g rel" % tuple(worst))
    assert worst[0] <= ORDER_FREE_SDF_ATOL and worst[1] <= ORDER_FREE_WEIGHT_RTOL


def _same_kfid_and_colour(a, b):
    ids = {tuple(x) for x in a.chunk_ids()}
    assert ids == {tuple(x) for x in b.chunk_ids()}
    for cid in sorted(ids):
        ca, cb = a.get_chunk(*cid), b.get_chunk(*cid)
        known = ca[1] > 0
        assert np.array_equal(known, cb[1] > 0)
        assert np.array_equal(ca[2], cb[2]), f"kfid of chunk {cid}: order-free against ordered"
        assert np.array_equal(ca[3][known], cb[3][known]), f"colour of chunk {cid}: order-free against ordered"


def _run(oracle, name, ordered_too=True, max_chunks=2048, after_call=None):
    from plvs_amd.tsdf import TsdfChisel
    sc = scene(name)
    grid = _grid(oracle, sc["width"])
    a = TsdfChisel(RES, max_chunks=max_chunks, order_free=True)      # depth entry
    b = TsdfChisel(RES, max_chunks=max_chunks, order_free=True)      # the oracle's clouds through the point-stream entry
    o = TsdfChisel(RES, max_chunks=max_chunks, order_free=False) if ordered_too else None
    for i, ((frames, kfids), (clouds, ref_map)) in enumerate(zip(sc["calls"], _reference(name))):
        _integrate_depth(a, frames, grid, STEP, MIN_DEPTH, sc["max_depth"], kfids)
        _integrate_clouds(b, clouds)
        assert a.last_stats()["visits"] == b.last_stats()["visits"] > 0
        assert compare_maps(a, b) >= 1
        _against_reference(a, ref_map)
        if o is not None:
            _integrate_depth(o, frames, grid, STEP, MIN_DEPTH, sc["max_depth"], kfids)
            _same_kfid_and_colour(a, o)
        if after_call is not None:
            after_call(i, a, kfids)
    for h in (a, b, o):
        if h is not None:
            h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["last_visitor_one_call", "last_visitor_two_calls"])
def test_last_visitor_across_images(oracle, name):
    def every_kfid_is_the_second_images(i, dev, kfids):
        if name == "last_visitor_two_calls" and i % 2 == 0:
            return
        last = kfids[-1]
        for cid in dev.chunk_ids():
            c = dev.get_chunk(*cid)
            assert (c[2][c[1] > 0] == last).all(), f"call {i}: a voxel of chunk {tuple(cid)} is not key frame {last}'s"
    _run(oracle, name, after_call=every_kfid_is_the_second_images)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_ray_per_voxel", "all_pixels"])
def test_one_ray_per_cold_voxel(oracle, name):
    _run(oracle, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["long_rays_7m", "short_rays_2m"])
def test_rays_longer_than_the_log(oracle, name):
    _run(oracle, name)


@pytest.mark.gpu
def test_tile_the_small_table_does_not_hold(oracle):
    """Two calls of 336 one-tile images.  The first (near walls, 2048-entry first pass: no tile beyond the small table) makes
    the small table the first pass of the second, in which 14 tiles see a wall 6 m away: more voxels than the small table
    takes, so walk_fast<1536> defers them and the list form of walk_fast<2048> walks them.  last_stats() does not tell a
    deferred tile from another: the check is the map."""
    _run(oracle, "tile_beyond_the_small_table", ordered_too=False, max_chunks=8192)
