"""The scenario of tests/test_tsdf_walk_small_table.py, run in a process of its own (PLVS_HIP_TSDF_TRACE is read once per
process): two order-free calls of three 640 x 480 stride-2 depth images (450 tiles: a call of more than 320 tiles takes the
lean plan) into a map of 3.5 cm voxels, through the depth entry and then, as the oracle's clouds, through the point-stream
entry.  Distinct voxels per 32 x 16 tile of grid pixels, from the geometry (every ray sampled at 161 points over its
truncation band, max(6 (0.0019 z^2 - 0.00152 z + 0.001504), 2 sqrt(3) voxels) either side of the surface):

  call 1  a frontal wall at 1.5 m: 140 - 200 voxels per tile, none beyond the small table — the handle's next first pass
          takes it
  call 2  a wall receding obliquely from 3 m to 4.9 m: 510 - 2 000 voxels per tile; about a quarter of the tiles hold more
          than the small table's 1 344 entries, a tenth more than the 1 792 of the 2 048-entry table behind it, none
          anywhere near the 3 584 of the largest.  (At 5 cm the same wall gives 250 - 800 voxels per tile: nothing to defer.)

The point-stream entry cuts the same points into strips of 512 consecutive points, 1.6 grid rows across the whole wall:
every strip of call 2 is beyond the small table, and most are beyond the next.

After every call the map is compared with the oracle's sequential integrate of the same clouds; one line
`<entry> call <k> chunks <n> sdf <worst> weight <worst>` per call goes to stdout."""
import sys

import numpy as np

RES = 0.035           # metres per voxel
SDF_ATOL = 2e-5       # metres, the order-free mode's stated tolerance (tests/test_tsdf_chisel.py)
WEIGHT_RTOL = 5e-5    # relative


def wall_frames(kind, seed):
    """Three images of a plane z = z0 + k x in the camera frame (k = 0: frontal), 2 mm of depth noise, random colours; the
    camera moves 2 cm between images."""
    from tests.plvs_amd_synth import TUM1
    rng = np.random.default_rng(seed)
    w, h = 640, 480
    xn = (np.arange(w, dtype=np.float64) - TUM1["cx"]) / TUM1["fx"]
    if kind == "frontal":
        z0, k = 1.5, 0.0
    else:   # 3 m at the left edge, 4.9 m at the right one (max_depth = 5 m is exclusive)
        lo, hi = xn[0], xn[-1]
        k = (4.9 - 3.0) / (4.9 * hi - 3.0 * lo)
        z0 = 3.0 * (1.0 - k * lo)
    z = np.broadcast_to(z0 / (1.0 - k * xn), (h, w))
    frames = []
    for i in range(3):
        Twc = np.eye(4, dtype=np.float32)[:3].copy()
        Twc[0, 3] = 0.02 * i
        frames.append(dict(depth=(z + 0.002 * rng.standard_normal((h, w))).astype(np.float32),
                           bgr=rng.integers(0, 256, (h, w, 3), dtype=np.uint8), Twc=Twc))
    return frames


def snapshot(ora):
    """The oracle's map as it stands: chunk id -> (sdf, weight, kfid, colour)."""
    return {tuple(int(v) for v in cid): tuple(np.array(p, copy=True) for p in ora.get_chunk(*cid)) for cid in ora.chunk_ids()}


def compare(want, dev, what):
    ids = set(want)
    assert ids == {tuple(int(v) for v in x) for x in dev.chunk_ids()}, f"{what}: the sets of chunks differ"
    worst = [0.0, 0.0]
    for cid in sorted(ids):
        a, b = want[cid], dev.get_chunk(*cid)
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
    return len(ids), worst


def main():
    import torch
    from plvs_amd.tsdf import TsdfChisel
    from tests import oracle_lib
    from tests.plvs_amd_synth import TUM1
    from tests.test_tsdf_chisel_depth import _clouds, _integrate_clouds, _integrate_depth

    oracle = oracle_lib.load()
    step = 2
    grid = oracle.cam_grid_points(640, 480, step, TUM1["fx"], TUM1["fy"], TUM1["cx"], TUM1["cy"])
    calls = [wall_frames("frontal", 1), wall_frames("oblique", 2)]
    kfids = [[10, 11, 12], [20, 21, 22]]
    clouds = [_clouds(oracle, fr, grid, step, 0.1, 5.0, kf) for fr, kf in zip(calls, kfids)]
    # the oracle's maps after call 1 and after call 2, once, for both entries
    ora = oracle.chisel(RES)
    want = []
    for cl in clouds:
        for c in cl:
            ora.integrate(c["xyz"], c["rgb"], c["kfid"], c["Twc"])
        want.append(snapshot(ora))
    for entry in ("depth", "clouds"):
        dev = TsdfChisel(RES, max_chunks=8192, order_free=True)
        for k, (fr, kf, cl) in enumerate(zip(calls, kfids, clouds)):
            if entry == "depth":
                _integrate_depth(dev, fr, grid, step, 0.1, 5.0, kf)
            else:
                _integrate_clouds(dev, cl)
            torch.cuda.synchronize()
            assert dev.last_stats()["visits"] > 0
            n, worst = compare(want[k], dev, f"{entry} call {k + 1}")
            print(f"{entry} call {k + 1} chunks {n} sdf {worst[0]:.3g} weight {worst[1]:.3g}", flush=True)
            assert worst[0] <= SDF_ATOL and worst[1] <= WEIGHT_RTOL, f"{entry} call {k + 1}: {worst}"
        dev.close()


if __name__ == "__main__":
    sys.exit(main())
