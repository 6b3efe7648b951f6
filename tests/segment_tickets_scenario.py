"""The scenes of tests/test_tsdf_segment_tickets.py, run in a process of their own: PLVS_TSDF_COLLECT and
PLVS_HIP_TSDF_TRACE are read once per process.  Every scene integrates into an order-free chisel map (5 cm) and into the CPU
oracle, and prints one JSON line: the SHA-256 of the whole map and of the updated-chunk list after every call, the stats,
and the worst deviations from the oracle.  Between two scenes a line `[scene] <name>` goes to stderr, where the library's
trace lines are."""
import hashlib
import json
import sys

import numpy as np


def map_hash(dev):
    h = hashlib.sha256()
    for cid in sorted(tuple(int(v) for v in c) for c in dev.chunk_ids()):
        h.update(np.asarray(cid, np.int32).tobytes())
        for plane in dev.get_chunk(*cid):
            h.update(np.ascontiguousarray(plane).tobytes())
    return h.hexdigest()


def updated_hash(dev):
    # (sorted: the list comes in pool-slot order, and which slot a new chunk gets is a race between the walk's tiles)
    ids = sorted(tuple(int(v) for v in c) for c in dev.updated_chunk_ids())
    return hashlib.sha256(np.asarray(ids, np.int32).tobytes()).hexdigest()


def against_oracle(ora, dev):
    """Worst sdf (m) and weight (relative) deviation over the observed voxels; kfid, colour and the observed set exact."""
    ia, ib = {tuple(x) for x in ora.chunk_ids()}, {tuple(x) for x in dev.chunk_ids()}
    out = dict(chunks=len(ia), same_chunks=ia == ib, exact=True, sdf=0.0, weight=0.0)
    for cid in sorted(ia & ib):
        a, b = ora.get_chunk(*cid), dev.get_chunk(*cid)
        known = a[1] > 0
        out["exact"] = bool(out["exact"] and np.array_equal(known, b[1] > 0) and np.array_equal(a[2], b[2])
                            and np.array_equal(a[3], b[3]))
        if known.any():
            out["sdf"] = max(out["sdf"], float(np.abs(a[0][known] - b[0][known]).max()))
            out["weight"] = max(out["weight"], float((np.abs(a[1][known] - b[1][known]) / a[1][known]).max()))
    return out


def wall_frames(n, depth, origin, seed):
    """A wall `depth` metres in front of a camera that looks along +z from `origin` and moves a few millimetres per frame."""
    rng = np.random.default_rng(seed)
    frames = []
    for k in range(n):
        d = (depth + 0.02 * rng.random((480, 640))).astype(np.float32)
        d[rng.random((480, 640)) < 0.03] = 0.0
        Twc = np.eye(4, dtype=np.float32)[:3].copy()
        Twc[:, 3] = np.asarray(origin, np.float32) + np.float32(0.004 * k)
        frames.append(dict(depth=d, bgr=rng.integers(0, 256, (480, 640, 3), dtype=np.uint8), Twc=Twc))
    return frames


def main():
    import torch
    from plvs_amd.tsdf import TsdfChisel
    from tests import oracle_lib
    from tests.plvs_amd_synth import TUM1, make_rgbd_frames
    from tests.test_tsdf_chisel import _scattered_cloud
    from tests.test_tsdf_chisel_depth import _clouds, _crop, _integrate_clouds, _integrate_depth

    oracle = oracle_lib.load()
    step = 2
    eye = np.eye(4, dtype=np.float32)[:3]

    def grid_of(w, h):
        return oracle.cam_grid_points(w, h, step, TUM1["fx"], TUM1["fy"], TUM1["cx"], TUM1["cy"])

    def depth_call(dev, ora, frames, grid, kf):
        _integrate_depth(dev, frames, grid, step, 0.1, 5.0, kf)
        torch.cuda.synchronize()
        if ora is not None:
            for c in _clouds(oracle, frames, grid, step, 0.1, 5.0, kf):
                ora.integrate(c["xyz"], c["rgb"], c["kfid"], c["Twc"])

    def cloud_call(dev, ora, cloud):
        xyz, rgb, kf = cloud
        _integrate_clouds(dev, [dict(xyz=xyz, rgb=rgb, kfid=kf, Twc=eye)])
        torch.cuda.synchronize()
        if ora is not None:
            ora.integrate(xyz, rgb, kf, eye)

    def report(name, dev, ora, **more):
        print(json.dumps(dict(scene=name, map=map_hash(dev), updated=updated_hash(dev), stats=dev.last_stats(),
                              n_updated=int(len({tuple(c) for c in dev.updated_chunk_ids()})),
                              oracle=against_oracle(ora, dev) if ora is not None else None, **more)), flush=True)

    def scene(name):
        print(f"[scene] {name}", file=sys.stderr, flush=True)

    # ---- small calls: one, then five key frames of 320 x 240 pixels (5 x 8 tiles each)
    small = _crop(make_rgbd_frames(6, seed=9, holes=True), 320, 240)
    small_grid = grid_of(320, 240)
    dev, ora = TsdfChisel(0.05, max_chunks=4096, order_free=True), oracle.chisel(0.05)
    scene("small_1")
    depth_call(dev, ora, small[:1], small_grid, [40])
    report("small_1", dev, ora)
    scene("small_5")
    depth_call(dev, ora, small[1:], small_grid, [41, 42, 43, 44, 45])
    report("small_5", dev, ora)
    dev.close()

    # ---- a busy chunk: five views of a wall 0.6 m away, all of it inside the chunk [0, 0.8 m)^3 — every tile of every
    # image (750) has a segment in that chunk
    busy = wall_frames(5, 0.6, (0.4, 0.4, 0.02), seed=4)
    full_grid = grid_of(640, 480)
    dev, ora = TsdfChisel(0.05, max_chunks=1024, order_free=True), oracle.chisel(0.05)
    scene("busy")
    depth_call(dev, ora, busy, full_grid, [50, 51, 52, 53, 54])
    report("busy", dev, ora)
    dev.close()

    # ---- tiles of the general kernel: points with no spatial coherence, a tile meets more chunks than its cache holds
    dev, ora = TsdfChisel(0.05, max_chunks=4096, order_free=True), oracle.chisel(0.05)
    scene("general")
    depth_call(dev, ora, small[:1], small_grid, [60])     # (not the handle's first call: its scratch has grown once)
    cloud_call(dev, ora, _scattered_cloud(700, 5, spread=2.0, zmax=3.0))
    report("general", dev, ora)
    dev.close()

    # ---- scratch retry: the first call of a fresh handle needs more spill room than the handle starts with
    dev, ora = TsdfChisel(0.05, max_chunks=16384, order_free=True), oracle.chisel(0.05)
    scene("retry")
    cloud_call(dev, ora, _scattered_cloud(3000, 1))
    report("retry", dev, ora, oracle_chunks=sorted(tuple(int(v) for v in c) for c in ora.chunk_ids()),
           updated_chunks=sorted(tuple(int(v) for v in c) for c in dev.updated_chunk_ids()))
    dev.close()

    # ---- the same three calls twice, on a cleared handle
    dev = TsdfChisel(0.05, max_chunks=4096, order_free=True)
    for rnd in (0, 1):
        dev.clear()
        scene(f"repeat_{rnd}")
        for i, call in enumerate((lambda: depth_call(dev, None, small[:1], small_grid, [70]),
                                  lambda: depth_call(dev, None, small[1:], small_grid, [71, 72, 73, 74, 75]),
                                  lambda: cloud_call(dev, None, _scattered_cloud(700, 5, spread=2.0, zmax=3.0)))):
            call()
            report(f"repeat_{rnd}_{i}", dev, None)
    dev.close()


if __name__ == "__main__":
    sys.exit(main())
