"""The projective depth + colour scan integrate on the GPU where the reference-made goldens end: against the CPU
restatement (tests/chisel_scan_restatement.py, itself pinned against the reference's own run by
tests/test_chisel_scan_reference.py) at full image size and at 2 cm far from the origin, the batch entry against single
calls, the capacity rule (chunks the reference would create and collect again take no slot), argument checks, row
pitches, and the PointCloudMapChisel front.  Every comparison is equality of bits."""
import json
import os

import numpy as np
import pytest

from tests import chisel_scan_scenario as S
from tests.chisel_scan_restatement import ScanIntegrator
from tests.synth_scene import TUM1, make_rgbd_frames

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chisel_scan_reference_digests.json")


def planes_equal(dev, store, what):
    ids = sorted(tuple(int(v) for v in c) for c in dev.chunk_ids())
    assert ids == sorted(store.ids()), f"{what}: chunk sets differ ({len(ids)} vs {len(store.ids())})"
    for cid in ids:
        for name, a, b in zip(("sdf", "weight", "kfid", "rgbw"), dev.get_chunk(*cid), store.get(cid)):
            assert np.array_equal(a.view(np.uint32), np.asarray(b).view(np.uint32)), f"{what}: chunk {cid}, plane {name}"
    return len(ids)


def push(frames, first):
    out = []
    for i, f in enumerate(frames):
        d = f["depth"].copy()
        if i >= first:
            h, w = d.shape
            d[h // 4:3 * h // 4, w // 4:3 * w // 4] += np.float32(0.6)
        out.append(dict(depth=d, bgr=f["bgr"], Twc=f["Twc"]))
    return out


def test_full_size_scans_match_the_restatement():
    """640 x 480, 5 cm, carving on, the third scan's centre pushed back so that voxels are reset; visits from the stats."""
    from plvs_amd.tsdf import TsdfChisel
    cam = dict(TUM1)
    frames = push(make_rgbd_frames(3, seed=31, holes=True), 2)
    r = ScanIntegrator(0.05, cam, 0.1, 5.0, carving=True)
    dev = TsdfChisel(0.05, max_chunks=4096)
    reset = 0
    for f in frames:
        st = r.integrate_scan(f["depth"], f["bgr"], f["Twc"])
        dev.integrate_scan(f["depth"], f["bgr"], cam, f["Twc"], near=0.1, far=5.0, use_carving=True)
        got = dev.last_stats()
        print("full size:", {k: st[k] for k in ("listed", "created", "kept", "integrated", "reset")}, got)
        assert got["visits"] == st["visits"] and got["points"] == 0 and got["new_chunks"] == st["kept"]
        assert got["updated_chunks"] == len(st["updated"])
        assert sorted(tuple(int(v) for v in c) for c in dev.updated_chunk_ids()) == sorted(st["updated"])
        reset += st["reset"]
    assert reset > 0 and planes_equal(dev, r.store, "full size") > 20
    dev.close()


def test_two_centimetres_far_from_the_origin():
    """2 cm voxels, the camera 300 m from the origin (chunk ids near 1000, coarse float coordinates)."""
    from plvs_amd.tsdf import TsdfChisel
    cam = S.cam()
    frames = make_rgbd_frames(2, cam=cam, seed=37, holes=True)
    for f in frames:
        f["Twc"] = f["Twc"].copy()
        f["Twc"][:, 3] += np.array([310.0, -205.0, 40.0], np.float32)
    r = ScanIntegrator(0.02, cam, 0.1, 3.0)
    dev = TsdfChisel(0.02, max_chunks=8192)
    for f in frames:
        st = r.integrate_scan(f["depth"], f["bgr"], f["Twc"])
        dev.integrate_scan(f["depth"], f["bgr"], cam, f["Twc"], near=0.1, far=3.0)
        assert dev.last_stats()["visits"] == st["visits"]
    n = planes_equal(dev, r.store, "2 cm")
    assert n > 50 and np.abs(dev.chunk_ids()).max() > 500
    dev.close()


def test_a_batch_of_25_is_25_single_calls():
    import torch
    from plvs_amd.tsdf import TsdfChisel
    cam = S.cam()
    frames = push(make_rgbd_frames(25, cam=cam, seed=41, holes=True), 12)
    one, batch = TsdfChisel(0.05, max_chunks=2048), TsdfChisel(0.05, max_chunks=2048)
    visits, updated = 0, set()
    for f in frames:
        one.integrate_scan(f["depth"], f["bgr"], cam, f["Twc"], use_carving=True)
        visits += one.last_stats()["visits"]
        updated |= {tuple(int(v) for v in c) for c in one.updated_chunk_ids()}
    batch.integrate_scans_dev(torch.from_numpy(np.stack([f["depth"] for f in frames])).cuda(),
                              torch.from_numpy(np.stack([f["bgr"] for f in frames])).cuda(), cam,
                              torch.from_numpy(np.stack([f["Twc"] for f in frames])).cuda(), use_carving=True)
    torch.cuda.synchronize()
    st = batch.last_stats()
    assert st["visits"] == visits and st["new_chunks"] == one.num_chunks() and st["points"] == 0
    assert {tuple(int(v) for v in c) for c in batch.updated_chunk_ids()} == updated

    class Single:
        def ids(self):
            return [tuple(int(v) for v in c) for c in one.chunk_ids()]

        def get(self, cid):
            return one.get_chunk(*cid)

    assert planes_equal(batch, Single(), "batch of 25") > 40
    one.close()
    batch.close()


def test_transient_chunks_take_no_capacity():
    """max_chunks = the final chunk count + 64, far below the chunks a scan lists (and the reference creates)."""
    import torch
    from plvs_amd.tsdf import TsdfChisel
    inp = S.inputs()
    cam = inp["cam"]
    r = ScanIntegrator(S.RES, cam, S.NEAR, S.FAR)
    listed = [r.integrate_scan(f["depth"], f["bgr"], f["Twc"])["listed"] for f in inp["frames"]]
    final = len(r.store.ids())
    assert min(listed) > 4 * (final + 64)
    for batch in (False, True):
        dev = TsdfChisel(S.RES, max_chunks=final + 64)
        if batch:
            dev.integrate_scans_dev(torch.from_numpy(np.stack([f["depth"] for f in inp["frames"]])).cuda(),
                                    torch.from_numpy(np.stack([f["bgr"] for f in inp["frames"]])).cuda(), cam,
                                    torch.from_numpy(np.stack([f["Twc"] for f in inp["frames"]])).cuda(), near=S.NEAR, far=S.FAR)
            torch.cuda.synchronize()
        else:
            for f in inp["frames"]:
                dev.integrate_scan(f["depth"], f["bgr"], cam, f["Twc"], near=S.NEAR, far=S.FAR)
        assert planes_equal(dev, r.store, "small pool") == final
        dev.close()


def test_order_free_and_sharded_handles_are_refused():
    import torch
    from plvs_amd import _lib
    from plvs_amd.tsdf import TsdfChisel
    cam = S.cam()
    f = make_rgbd_frames(1, cam=cam, seed=43)[0]
    for kw in (dict(order_free=True), dict(shard_rank=0, shard_count=2)):
        dev = TsdfChisel(0.05, max_chunks=256, **kw)
        with pytest.raises(Exception) as e:
            dev.integrate_scan(f["depth"], f["bgr"], cam, f["Twc"])
        assert "invalid argument" in str(e.value)
        with pytest.raises(Exception) as e:
            dev.integrate_scans_dev(torch.from_numpy(f["depth"][None]).cuda(), torch.from_numpy(f["bgr"][None]).cuda(), cam,
                                    torch.from_numpy(f["Twc"][None]).cuda())
        assert "invalid argument" in str(e.value)
        assert dev.num_chunks() == 0
        dev.close()
    # no colour image: refused as well (the depth-only integrator is not provided)
    dev = TsdfChisel(0.05, max_chunks=256)
    c = _lib_scan_camera(cam)
    fn = _lib.lib.plvs_hip_tsdf_chisel_integrate_scan
    import ctypes
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float]
    rc = fn(dev._h, _lib.np_ptr(f["depth"]), f["depth"].strides[0], None, 0, 3, ctypes.byref(c), _lib.np_ptr(f["Twc"]), 0, 0.05)
    assert rc == _lib.PLVS_ERR_INVALID_ARG and dev.num_chunks() == 0
    dev.close()


def _lib_scan_camera(cam):
    from plvs_amd.tsdf import ScanCamera
    return ScanCamera.of(cam, 0.1, 5.0)


def test_row_pitches():
    """Rows further apart than width x element size (a cv::Mat region of interest): the same map."""
    from plvs_amd.tsdf import TsdfChisel
    cam = S.cam()
    frames = make_rgbd_frames(2, cam=cam, seed=47, holes=True)
    h, w = frames[0]["depth"].shape
    dense, strided = TsdfChisel(0.05, max_chunks=1024), TsdfChisel(0.05, max_chunks=1024)
    for f in frames:
        dense.integrate_scan(f["depth"], f["bgr"], cam, f["Twc"])
        big_d = np.full((h, w + 13), np.float32(1.0))
        big_c = np.full((h, w + 5, 3), 77, np.uint8)
        big_d[:, :w] = f["depth"]
        big_c[:, :w] = f["bgr"]
        d, c = big_d[:, :w], big_c[:, :w]
        assert d.strides[0] == (w + 13) * 4 and c.strides[0] == (w + 5) * 3
        strided.integrate_scan(d, c, cam, f["Twc"])
        assert strided.last_stats() == dense.last_stats()

    class Dense:
        def ids(self):
            return [tuple(int(v) for v in c) for c in dense.chunk_ids()]

        def get(self, cid):
            return dense.get_chunk(*cid)

    assert planes_equal(strided, Dense(), "row pitches") > 8
    dense.close()
    strided.close()


def test_insert_data_then_update_map_gives_the_golden_mesh(capsys):
    from plvs_amd.tsdf import PointCloudMapChisel
    with open(GOLDEN) as fh:
        g = json.load(fh)
    inp = S.inputs()
    assert S.inputs_digest(inp) == g["inputs"]
    cam = inp["cam"]
    m = PointCloudMapChisel(S.RES, min_depth=S.NEAR, max_depth=S.FAR)
    m.SetDepthCameraModel(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"])
    m.InsertData(dict(type="kColorAndDepthImages", imgDepth=np.zeros((0, 0), np.float32), imgColor=inp["frames"][0]["bgr"],
                      Twc=inp["frames"][0]["Twc"]))
    assert "ERROR: depth and/or color images are emtpy" in capsys.readouterr().out and m.tsdf.num_chunks() == 0
    for f in inp["frames"]:
        m.InsertData(dict(type="kColorAndDepthImages", imgDepth=f["depth"], imgColor=f["bgr"], Twc=f["Twc"], timestamp=1))
    cloud = m.UpdateMap()
    want = g["stages"]["plain"][-1]
    empty = (np.zeros((0, 3), np.float32),) * 3 + (np.zeros(0, np.uint32),)

    def mesh_of(*cid):
        e = m.all_meshes.get(tuple(cid))
        return empty if e is None else (e["vertices"], e["normals"], e["colors"], e["kfids"])

    ids = [tuple(int(v) for v in c) for c in m.tsdf.chunk_ids()]
    assert set(m.all_meshes) <= set(ids), "a mesh for a chunk the map does not have"
    got = S.mesh_digest(ids, mesh_of)
    assert got == {k: want[k] for k in ("vertices", "mesh")} and len(cloud) == want["vertices"] > 1000
    assert S.map_digest(ids, m.tsdf.get_chunk) == {k: want[k] for k in ("chunks", "planes")}
    with pytest.raises(SystemExit):                    # other unknown kinds keep terminating
        m.InsertData(dict(type="kSomethingElse", Twc=inp["frames"][0]["Twc"]))
