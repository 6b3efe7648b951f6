"""The ordered integrate and depth-image carving of the HIP chisel map under cameras with roll and pitch
(tests/camera_attitudes.py), against the CPU oracle, bit for bit.  The cases are those of
tests/test_oracle_pinned_chisel_map.py, where the reference's own compiled library pins the oracle on them: with the
yaw-only poses of every other TSDF test no row of R^T (c - t), no frustum corner and no plane distance ever sums three
non-zero products."""
import numpy as np
import pytest

from tests.test_oracle_pinned_chisel_map import attitude_keyframes, carving_cases, small_cam
from tests.test_tsdf_chisel import compare_maps

pytestmark = pytest.mark.gpu


def test_ordered_integrate_under_roll_and_pitch_matches_the_oracle(oracle):
    from plvs_amd.tsdf import TsdfChisel
    cam = small_cam(4)
    ora, dev = oracle.chisel(0.05), TsdfChisel(0.05, max_chunks=1024)
    for kf in attitude_keyframes(cam):
        ora.integrate(kf["xyz"], kf["rgb"], kf["kfid"], kf["Twc"])
        dev.integrate(kf["xyz"], kf["rgb"], kf["kfid"], kf["Twc"])
        assert dev.last_stats()["visits"] == ora.last_visits(), kf["name"]
        compare_maps(ora, dev)
    assert compare_maps(ora, dev) > 50
    dev.close()


def test_carving_under_roll_and_pitch_with_edge_depths_and_seeded_voxels_matches_the_oracle(oracle):
    """+-inf, negative, -0.0, 0, 1e-6, NaN and 25.0 patches on chunks seeded at the edges of `weight <= 1e-15` and
    `sdf < 1e-5` (both compared in double), then every attitude carving what the others integrated: the carved-chunk
    count and ids of every call, and the map after it."""
    from plvs_amd.tsdf import TsdfChisel
    cam, chunks, steps = carving_cases()
    ora, dev = oracle.chisel(0.05), TsdfChisel(0.05, max_chunks=1024)
    for cid, planes in chunks:
        ora.set_chunk(*cid, *planes)
        dev.set_chunk(*cid, *planes)
    compare_maps(ora, dev)
    carved = []
    for kf, depth in steps:
        want_n, want_ids = ora.carve(depth, cam["fx"], cam["fy"], cam["cx"], cam["cy"], kf["Twc"])
        got_n = dev.carve(depth, cam["fx"], cam["fy"], cam["cx"], cam["cy"], kf["Twc"])
        assert got_n == want_n, kf["name"]
        assert {tuple(i) for i in dev.updated_chunk_ids()} == {tuple(i) for i in want_ids}, kf["name"]
        compare_maps(ora, dev)
        carved.append(want_n)
        ora.integrate(kf["xyz"], kf["rgb"], kf["kfid"], kf["Twc"])
        dev.integrate(kf["xyz"], kf["rgb"], kf["kfid"], kf["Twc"])
        compare_maps(ora, dev)
    assert carved[0] > 0 and sum(c > 0 for c in carved[5:]) >= 4, carved
    assert not any(np.isnan(dev.get_chunk(*c)[0]).any() for c in dev.chunk_ids())
    dev.close()
