"""The voxblox handle's refusals and failures (plvs_hip_tsdf_voxblox_*): a full block pool poisons the handle until clear(),
the three phases of the ray-sharded step come in their order, a batch with bad offsets is refused and leaves the map alone.
Every case is a designed error return (code + text) of the C ABI; the maps around them are compared with the CPU oracle bit
for bit."""
import numpy as np
import pytest

from tests.plvs_amd_synth import make_keyframes
from tests.test_tsdf_voxblox import compare, rgba_of, small_cam
from tests.test_tsdf_voxblox_shard import _batch, sharded_step

IDENTITY = np.eye(4, dtype=np.float32)[:3]
TINY_XYZ = np.array([[0.011, 0.017, 1.0], [0.02, 0.03, 1.02], [-0.01, 0.02, 0.98]], np.float32)
TINY_RGBA = np.array([[200, 40, 10, 255], [30, 220, 60, 255], [90, 90, 250, 255]], np.uint8)
TINY = (TINY_XYZ, TINY_RGBA, IDENTITY)


def _raises(code, text, call, *args):
    from plvs_amd import _lib
    with pytest.raises(_lib.PlvsHipError) as e:
        call(*args)
    assert e.value.code == code, str(e.value)
    assert text in str(e.value)


@pytest.mark.gpu
def test_hip_full_pool_poisons_the_handle_until_clear(oracle):
    import torch
    from plvs_amd import _lib
    from plvs_amd.tsdf import TsdfVoxblox
    kf = make_keyframes(1, cam=small_cam(4), seed=23)[0]
    ora_tiny, ora_kf = oracle.voxblox(0.05), oracle.voxblox(0.05)
    ora_tiny.integrate(*TINY)
    ora_kf.integrate(kf["xyz"], rgba_of(kf), kf["Twc"])
    assert len(ora_kf.chunk_ids()) > 4 >= len(ora_tiny.chunk_ids())
    dev = TsdfVoxblox(0.05, max_blocks=4)
    dev.integrate(*TINY)
    assert compare(ora_tiny, dev) == len(ora_tiny.chunk_ids())
    _raises(_lib.PLVS_ERR_CAPACITY, "block pool full", dev.integrate, kf["xyz"], rgba_of(kf), kf["Twc"])
    normals = np.tile(np.array([[0.0, 0.0, -1.0]], np.float32), (3, 1))
    d_xyz, d_Twc = torch.from_numpy(TINY_XYZ).cuda(), torch.from_numpy(IDENTITY[None]).cuda()
    for call, args in ((dev.integrate, TINY), (dev.integrate_fast, TINY), (dev.integrate_merged, TINY),
                       (dev.integrate_world_normals, (TINY_XYZ, TINY_RGBA, normals)),
                       (dev.shard_walk, (d_xyz, np.array([0, 3], np.int32), d_Twc))):
        _raises(_lib.PLVS_ERR_INVALID_ARG, "failed state", call, *args)
    dev.clear()
    assert dev.num_chunks() == 0
    dev.integrate(*TINY)
    dev.integrate_fast(*TINY)
    ora = oracle.voxblox(0.05)
    ora.integrate(*TINY)
    ora.integrate_fast(*TINY, approx_sets=True)
    assert compare(ora, dev) == len(ora.chunk_ids())
    dev.close()


@pytest.mark.gpu
def test_hip_sharded_step_phases_come_in_order():
    import torch
    from plvs_amd import _lib
    from plvs_amd.tsdf import TsdfVoxblox
    xyz, rgba, offsets, Twc = _batch(make_keyframes(2, cam=small_cam(4), seed=23))
    dev = TsdfVoxblox(0.05, max_blocks=8192, shard_count=1)
    none = torch.zeros((0, 4), dtype=torch.int32, device="cuda")
    apply_nothing = (none, np.zeros(1, np.int64), xyz, rgba, offsets, Twc)
    _raises(_lib.PLVS_ERR_INVALID_ARG, "shard_pack follows shard_walk", dev.shard_pack, none)
    _raises(_lib.PLVS_ERR_INVALID_ARG, "shard_apply follows shard_pack", dev.shard_apply, *apply_nothing)
    counts = dev.shard_walk(xyz, offsets, Twc)
    assert counts.sum() > 0
    _raises(_lib.PLVS_ERR_INVALID_ARG, "shard_apply follows shard_pack", dev.shard_apply, *apply_nothing)
    send = torch.zeros((int(counts.sum()), 4), dtype=torch.int32, device="cuda")
    dev.shard_pack(send)
    dev.shard_apply(send, counts, xyz, rgba, offsets, Twc)
    torch.cuda.synchronize()
    single = TsdfVoxblox(0.05, max_blocks=8192)
    single.integrate_batch_dev(xyz, rgba, offsets, Twc)
    torch.cuda.synchronize()
    assert compare(single, dev) > 4
    # and the step as the sharded tests drive it, on the populated maps
    sharded_step([dev], xyz, rgba, offsets, Twc)
    single.integrate_batch_dev(xyz, rgba, offsets, Twc)
    torch.cuda.synchronize()
    compare(single, dev)
    dev.close()
    single.close()


@pytest.mark.gpu
def test_hip_refused_batch_leaves_the_map(oracle):
    import torch
    from plvs_amd import _lib
    from plvs_amd.tsdf import TsdfVoxblox
    dev = TsdfVoxblox(0.05, max_blocks=64)
    dev.integrate(*TINY)
    five = torch.from_numpy(np.concatenate([TINY_XYZ, TINY_XYZ[:2]])).cuda()
    five_rgba = torch.from_numpy(np.concatenate([TINY_RGBA, TINY_RGBA[:2]])).cuda()
    two_poses = torch.from_numpy(np.stack([IDENTITY, IDENTITY])).cuda()
    _raises(_lib.PLVS_ERR_INVALID_ARG, "non-decreasing", dev.integrate_batch_dev, five, five_rgba, np.array([0, 5, 3], np.int32),
            two_poses)
    dev.integrate(*TINY)   # (not poisoned)
    ora = oracle.voxblox(0.05)
    ora.integrate(*TINY)
    ora.integrate(*TINY)
    assert compare(ora, dev) == len(ora.chunk_ids())
    dev.close()
