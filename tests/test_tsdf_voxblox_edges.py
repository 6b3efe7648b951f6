"""The voxblox back end on the device OFF the defaults (tests/voxblox_edge_scenario.py): truncation, ray gates and carving
other than PointCloudMapVoxblox's, poses up to 30 km from the origin, the degenerate cloud (depth zero, axis-aligned rays,
voxel corners, repeated points), and the edge of the block range a map accepts.  Bar: the oracle's map bit for bit —
block set, distance and weight WORDS (a NaN must be the same NaN), colours, visit counts.  The oracle itself is pinned on
the same inputs by the reference's compiled integrators (tests/test_oracle_pinned_voxblox_edges.py)."""
import numpy as np
import pytest

from tests import voxblox_edge_scenario as sc
from tests.test_tsdf_voxblox import compare

pytestmark = pytest.mark.gpu

_IDS = lambda p: "v%g_t%g_r%g-%g_c%d" % p
METHODS = ["integrate", "batch", "merged", "fast"]


def _oracle_map(oracle, pset, **kw):
    voxel, trunc, min_ray, max_ray, carving = pset
    return oracle.voxblox(voxel, truncation=trunc, min_ray=min_ray, max_ray=max_ray, carving=bool(carving), **kw)


def _device_map(pset, **kw):
    from plvs_amd.tsdf import TsdfVoxblox
    voxel, trunc, min_ray, max_ray, carving = pset
    return TsdfVoxblox(voxel, use_carving=bool(carving), max_blocks=8192, truncation=trunc, min_ray_length=min_ray,
                       max_ray_length=max_ray, **kw)


def _batch(clouds):
    import torch
    xyz = torch.from_numpy(np.concatenate([c[0] for c in clouds])).cuda()
    rgba = torch.from_numpy(np.concatenate([c[1] for c in clouds])).cuda()
    Twc = torch.from_numpy(np.stack([c[2] for c in clouds])).cuda()
    offsets = np.cumsum([0] + [len(c[0]) for c in clouds]).astype(np.int32)
    return xyz, rgba, offsets, Twc


def _run(method, ora, dev, clouds):
    """One round of `clouds` through the oracle and the device by `method`; the visit counts must agree call by call."""
    import torch
    if method == "batch":                       # both clouds in ONE device call; the oracle takes them one after the other
        visits = 0
        for c in clouds:
            ora.integrate(*c)
            visits += ora.last_visits()
        dev.integrate_batch_dev(*_batch(clouds))
        torch.cuda.synchronize()
        assert dev.last_stats()["visits"] == visits
        return visits
    visits = 0
    for c in clouds:
        if method == "merged":
            ora.integrate_merged(*c)
            dev.integrate_merged(*c)
        elif method == "fast":
            ora.integrate_fast(*c, approx_sets=True)
            dev.integrate_fast(*c)
        else:
            ora.integrate(*c)
            dev.integrate(*c)
        assert dev.last_stats()["visits"] == ora.last_visits()
        visits += ora.last_visits()
    return visits


def _check(oracle, pset, method, clouds0, offsets):
    dev = _device_map(pset)
    visits = 0
    for offset in offsets:
        clouds = sc.shifted(clouds0, offset)
        ora = _oracle_map(oracle, pset)
        dev.clear()
        visits += _run(method, ora, dev, clouds)
        assert compare(ora, dev) > 0, offset
        visits += _run(method, ora, dev, clouds[::-1])       # a second call on the populated map
        compare(ora, dev)
    dev.close()
    return visits


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pset", sc.PARAM_SETS, ids=_IDS)
def test_hip_keyframe_clouds_off_the_defaults_and_far_from_the_origin(oracle, pset, method):
    assert _check(oracle, pset, method, sc.keyframe_clouds(), sc.OFFSETS) > 1000


@pytest.mark.parametrize("method", ["integrate", "batch", "fast"])
@pytest.mark.parametrize("pset", sc.DEGENERATE_SETS, ids=_IDS)
def test_hip_degenerate_cloud(oracle, pset, method):
    """Depth zero (weight 0; behind the drop-off's zero crossing a weight of -0.0 or a sign-set NaN, which must not
    disturb the end-of-run mark vb_expand keeps in the weight's sign bit: as a voxel's only record, inside and at the
    end of runs of 16 and more — test_degenerate_cloud_feeds_the_fold_weights_that_carry_a_sign_bit shows they are
    there), a drop-off denominator of zero (NaN and infinite weights), axis-aligned rays that never advance, points on
    voxel corners, both sides of the range gates."""
    clouds = sc.degenerate_clouds(pset[0], pset[2], pset[3])
    assert _check(oracle, pset, method, clouds, sc.DEGENERATE_OFFSETS) > 1000


@pytest.mark.parametrize("pset", sc.DEGENERATE_SETS, ids=_IDS)
def test_hip_merged_on_the_degenerate_cloud_without_its_weightless_points(oracle, pset):
    """integrate_merged (vb_merge_keys, vb_merge_bundles, the merged flavour of the ray passes and of vb_expand) on the
    degenerate cloud less the points of weight 0, which the reference cannot bundle (next test): axis-aligned rays,
    voxel corners, both sides of the range gates, a hundred points in one bundle, clearing bundles, the zero and
    negative drop-off denominators."""
    clouds = sc.degenerate_clouds(pset[0], pset[2], pset[3], weightless=False)
    assert _check(oracle, pset, "merged", clouds, sc.DEGENERATE_OFFSETS) > 1000


@pytest.mark.parametrize("d0,w0", [(-0.0, 1.0), (0.05, -0.0)], ids=["distance_minus_zero", "weight_minus_zero"])
def test_hip_zero_weight_visit_on_a_voxel_of_distance_minus_zero(oracle, d0, w0):
    """The one place where the sign of a zero weight reaches the map: (sdf * uw + D * W) / (W + uw) with D = -0.0.  The
    reference's uw = -0.0 makes the sum +0.0, a weight of +0.0 in its place -0.0.  Blocks uploaded with distance -0.0
    and weight 1, then the degenerate cloud: the oracle's words, the sign of every zero distance included.  And blocks
    uploaded with a WEIGHT of -0.0: the fold's eight-lane path marks a skipped visit in the sign of the weight before it."""
    from tests.test_tsdf_voxblox_mesh import set_block
    pset = sc.PARAM_SETS[0]
    clouds = sc.degenerate_clouds(pset[0], pset[2], pset[3])
    probe = _oracle_map(oracle, pset)
    for c in clouds:
        probe.integrate(*c)
    ora, dev = _oracle_map(oracle, pset), _device_map(pset)
    d, w, c0 = np.full(4096, d0, np.float32), np.full(4096, w0, np.float32), np.zeros(4096, np.uint32)
    for bid in probe.chunk_ids():
        set_block(ora, *bid, d, w, c0)
        dev.set_chunk(*bid, d, w, c0)
    for c in clouds:
        ora.integrate(*c)
        dev.integrate(*c)
        assert dev.last_stats()["visits"] == ora.last_visits()
    assert dev.last_stats()["max_run"] >= 100
    assert compare(ora, dev) == len(probe.chunk_ids())
    if w0 == 1.0:
        turned = sum(int(((ora.get_chunk(*b)[0].view(np.uint32) == 0) & (ora.get_chunk(*b)[1] == 1)).sum()) for b in ora.chunk_ids())
        assert turned >= 10, "voxels whose only visits had weight -0.0: distance -0.0 became +0.0, the weight stayed 1"
    dev.close()


@pytest.mark.parametrize("pset", sc.DEGENERATE_SETS[:2], ids=_IDS)
def test_hip_merged_refuses_a_bundle_of_weightless_points(oracle, pset):
    """MergedTsdfIntegrator's bundle of z = 0 points alone has weight 0 and the merged point 0 / 0 (tsdf_integrator.cc:
    404-416); the reference casts a ray to voxel index (int)NaN.  The device refuses the call as it refuses a non-finite
    point; clear() revives the handle."""
    from plvs_amd import _lib
    dev = _device_map(pset)
    cloud = sc.degenerate_clouds(pset[0], pset[2], pset[3])[0]
    with pytest.raises(_lib.PlvsHipError) as e:
        dev.integrate_merged(*cloud)
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and "non-finite" in str(e.value)
    dev.clear()
    kf = sc.keyframe_clouds()[0]
    ora = _oracle_map(oracle, pset)
    ora.integrate_merged(*kf)
    dev.integrate_merged(*kf)
    assert compare(ora, dev) > 0
    dev.close()


def test_hip_block_range_edge_is_exact_and_one_block_further_is_refused(oracle):
    """A map accepts block ids in [-2^19, 2^19): there the binary32 voxel centre of visit_operands is the reference's
    (double 0.5, one rounding).  Blocks 2^19 - 1 and -2^19 are bit-exact; one block further the call fails with
    PLVS_ERR_CAPACITY, the handle stays failed until clear()."""
    import torch
    from plvs_amd import _lib
    pset = sc.PARAM_SETS[0]
    inside, outside = sc.range_edge_clouds(pset[0]), sc.range_edge_clouds(pset[0], shift_blocks=1)
    ora, dev = _oracle_map(oracle, pset), _device_map(pset)
    for c in inside:
        ora.integrate(*c)
        dev.integrate(*c)
        assert dev.last_stats()["visits"] == ora.last_visits() > 0
    ids = ora.chunk_ids()
    assert ids[:, 0].max() == sc.BLOCK_LIMIT - 1 and ids[:, 1].min() == -sc.BLOCK_LIMIT
    assert compare(ora, dev) == len(ids)

    def raises(code, text, call, *args):
        with pytest.raises(_lib.PlvsHipError) as e:
            call(*args)
        assert e.value.code == code and text in str(e.value), str(e.value)

    for k, c in enumerate(outside):
        raises(_lib.PLVS_ERR_CAPACITY, "block id outside [-2^19, 2^19)", dev.integrate, *c)
        d_xyz, _, offsets, d_Twc = _batch([inside[0]])
        normals = np.tile(np.array([[0.0, 0.0, -1.0]], np.float32), (len(inside[0][0]), 1))
        for call, args in ((dev.integrate, inside[0]), (dev.integrate_fast, inside[0]), (dev.integrate_merged, inside[0]),
                           (dev.integrate_world_normals, (inside[0][0], inside[0][1], normals)),
                           (dev.shard_walk, (d_xyz, offsets, d_Twc))):
            raises(_lib.PLVS_ERR_INVALID_ARG, "failed state", call, *args)
        dev.clear()
        assert dev.num_chunks() == 0
        again = _oracle_map(oracle, pset)
        again.integrate(*inside[k])
        dev.integrate(*inside[k])
        assert compare(again, dev) == len(again.chunk_ids())
    # the other two ways into the directory: the ray-sharded walk (it only reads the clouds: the handle stays usable) and
    # upload_block
    d_xyz, _, offsets, d_Twc = _batch([outside[1]])
    raises(_lib.PLVS_ERR_CAPACITY, "block id outside [-2^19, 2^19)", dev.shard_walk, d_xyz, offsets, d_Twc)
    dev.integrate(*inside[0])
    zeros = np.zeros(4096, np.float32)
    dev.set_chunk(sc.BLOCK_LIMIT - 1, 0, -sc.BLOCK_LIMIT, zeros, zeros, zeros.view(np.uint32))
    raises(_lib.PLVS_ERR_CAPACITY, "block id outside [-2^19, 2^19)", dev.set_chunk, 0, sc.BLOCK_LIMIT, 0, zeros, zeros,
           zeros.view(np.uint32))
    torch.cuda.synchronize()
    dev.close()


def test_hip_mesh_blocks_far_from_the_origin(oracle):
    """mesh_blocks reads the directory with large and negative block ids: against the oracle's mesher."""
    from tests.test_tsdf_voxblox_mesh import mesh_block
    pset = sc.PARAM_SETS[0]
    ora, dev = _oracle_map(oracle, pset), _device_map(pset)
    for c in sc.shifted(sc.keyframe_clouds(), sc.FAR_OFFSET):
        ora.integrate(*c)
        dev.integrate(*c)
    ids = sorted(tuple(int(x) for x in b) for b in ora.chunk_ids())
    assert ids == sorted(tuple(int(x) for x in b) for b in dev.chunk_ids())
    assert min(b[0] for b in ids) < -200 and max(b[1] for b in ids) > 600 and min(b[2] for b in ids) < -100
    m = dev.mesh_blocks(np.array(ids, np.int32))
    first, total = m["block_first"], 0
    for i, bid in enumerate(ids):
        v, n, c = mesh_block(ora, *bid)
        a, b = int(first[i]), int(first[i + 1])
        assert b - a == len(v), (bid, b - a, len(v))
        assert m["vertices"][a:b].tobytes() == v.tobytes(), bid
        assert m["normals"][a:b].tobytes() == n.tobytes(), bid
        assert m["colors"][a:b].tobytes() == c.tobytes(), bid
        total += len(v)
    assert total == len(m["vertices"]) and total > 300
    dev.close()


def test_hip_ray_sharded_integrate_far_from_the_origin(oracle):
    """The ray-sharded integrate on three virtual ranks at an offset with negative block ids: owner_hash sign-extends
    them; every rank's shard is the oracle's shard bit for bit."""
    from tests.test_tsdf_voxblox_shard import sharded_step
    pset, world = sc.PARAM_SETS[0], 3
    clouds = sc.shifted(sc.keyframe_clouds(), sc.FAR_OFFSET)
    ranks = [_device_map(pset, shard_rank=r, shard_count=world) for r in range(world)]
    oras = [_oracle_map(oracle, pset, shard_rank=r, shard_count=world) for r in range(world)]
    whole = _oracle_map(oracle, pset)
    visits = 0
    for c in clouds:
        whole.integrate(*c)
        visits += whole.last_visits()
        for o in oras:
            o.integrate(*c)
    counts = sharded_step(ranks, *_batch(clouds))
    assert int(sum(c.sum() for c in counts)) == visits == sum(t.last_stats()["visits"] for t in ranks)
    blocks = [compare(o, t) for o, t in zip(oras, ranks)]
    assert sum(blocks) == len(whole.chunk_ids()) and min(blocks) > 0
    for t in ranks:
        t.close()


def test_hip_world_normals_with_a_wide_truncation_far_from_the_origin(oracle):
    """integrate_world_normals (the LoadMap path) casts point + n * truncation -> point - n * truncation: with
    truncation 0.2 instead of the default, far from the origin, onto a map with camera-ray history."""
    from tests.test_tsdf_loadmap import surface_cloud
    pset = sc.PARAM_SETS[1]
    ora, dev = _oracle_map(oracle, pset), _device_map(pset)
    for c in sc.shifted(sc.keyframe_clouds(), sc.FAR_OFFSET):
        ora.integrate(*c)
        dev.integrate(*c)
    # (the cloud itself lies far out, the pose is the identity as in LoadMap: integrateWorlPointCloud applies the FULL
    # transformation to the normal, so a far pose translation would make every ray hundreds of metres long)
    xyz, rgb, _, nrm = surface_cloud(3000, 7, pset[0])
    xyz = (xyz.astype(np.float64) + np.array(sc.FAR_OFFSET)).astype(np.float32)
    rgba = np.concatenate([rgb, np.full((len(rgb), 1), 200, np.uint8)], 1)
    ora.integrate_world_normals(xyz, rgba, nrm)
    dev.integrate_world_normals(xyz, rgba, nrm)
    assert dev.last_stats()["visits"] == ora.last_visits() > 10000
    assert compare(ora, dev) > 10
    dev.close()
