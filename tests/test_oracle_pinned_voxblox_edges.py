"""The voxblox oracle pinned by the reference's own compiled integrators (oracle/_ref/libvoxblox_ref.so, as
tests/test_oracle_pinned.py) OFF the defaults: truncation, ray gates and carving of tests/voxblox_edge_scenario.py, poses
up to 30 km out and across voxel index +-2^23, and the degenerate cloud (depth zero, axis-aligned rays, voxel corners,
repeated points).  reference == oracle == host build of the device arithmetic (hostvbx) for "simple", reference == oracle
for "merged" and "fast", every voxel of every block, bit for bit.

What the far poses found: the reference forms a voxel's centre with a double 0.5 (common.h:179-184: binary64 sum and
product, one rounding); in binary32 it is the same float only for |voxel index| < 2^23.  The oracle now follows the
reference; the device keeps binary32 and accepts block ids in [-2^19, 2^19) only, so hostvbx is compared inside that range."""
import ctypes
import os

import numpy as np
import pytest

from tests import oracle_lib
from tests import voxblox_edge_scenario as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VREF = os.path.join(ROOT, "oracle", "_ref", "libvoxblox_ref.so")

_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(VREF):
        pytest.skip("oracle/_ref/libvoxblox_ref.so not present")
    lib = ctypes.CDLL(VREF)
    lib.ref_voxblox_create.restype = _vp
    lib.ref_voxblox_create.argtypes = [_f] * 5 + [_i, ctypes.c_char_p]
    lib.ref_voxblox_integrate.argtypes = [_vp] * 5 + [_i]
    lib.ref_voxblox_destroy.argtypes = [_vp]
    lib.ref_voxblox_num_blocks.argtypes = [_vp]
    lib.ref_voxblox_block_ids.argtypes = [_vp, _vp]
    lib.ref_voxblox_get_block.argtypes = [_vp] + [_i] * 3 + [_vp] * 3
    return lib


@pytest.fixture(scope="module")
def oracle():
    o = oracle_lib.load()
    o.lib.oracle_voxblox_pose_quat.argtypes = [_vp, _vp]
    return o


def _ref_run(ref, oracle, pset, method, clouds):
    voxel, trunc, min_ray, max_ray, carving = pset
    h = _vp(ref.ref_voxblox_create(voxel, trunc, 10000.0, min_ray, max_ray, int(carving), method.encode()))
    for xyz, rgba, Twc in clouds:
        q = np.zeros(4, np.float32)
        oracle.lib.oracle_voxblox_pose_quat(Twc.ctypes.data, q.ctypes.data)
        t = np.ascontiguousarray(Twc[:, 3])
        ref.ref_voxblox_integrate(h, q.ctypes.data, t.ctypes.data, xyz.ctypes.data, rgba.ctypes.data, len(xyz))
    n = ref.ref_voxblox_num_blocks(h)
    ids = np.zeros((max(n, 1), 3), np.int32)
    ref.ref_voxblox_block_ids(h, ids.ctypes.data)
    out = {}
    for b in ids[:n]:
        d, w, c = np.zeros(4096, np.float32), np.zeros(4096, np.float32), np.zeros(4096, np.uint32)
        assert ref.ref_voxblox_get_block(h, int(b[0]), int(b[1]), int(b[2]), d.ctypes.data, w.ctypes.data, c.ctypes.data)
        out[tuple(int(v) for v in b)] = (d, w, c)
    ref.ref_voxblox_destroy(h)
    return out


def _like(lib, prefix, pset):
    voxel, trunc, min_ray, max_ray, carving = pset
    return oracle_lib._VoxbloxLike(lib, prefix, voxel, truncation=trunc, min_ray=min_ray, max_ray=max_ray, carving=bool(carving))


def _blocks(m):
    return {tuple(int(v) for v in b): m.get_chunk(*b) for b in m.chunk_ids()}


def _assert_equal(want, got, what):
    assert set(got) == set(want), (what, len(want), len(got))
    for bid, planes in want.items():
        for name, x, y in zip(("distance", "weight", "colour"), planes, got[bid]):   # words: a NaN must be the same NaN
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, name, bid, int((x.view(np.uint32) != y.view(np.uint32)).sum()))


def _integrate(m, method, clouds):
    for c in clouds:
        if method == "merged":
            m.integrate_merged(*c)
        elif method == "fast":
            m.integrate_fast(*c, approx_sets=True)
        else:
            m.integrate(*c)


def _clouds_of(kind, pset):
    if kind == "keyframes":
        return sc.keyframe_clouds()
    return sc.degenerate_clouds(pset[0], pset[2], pset[3], weightless=(kind == "degenerate"))


def _straddles(ids, offset, limit=sc.BLOCK_LIMIT):
    """Do the block ids lie on both sides of +-2^19 on every axis the offset moves?"""
    ids = np.array(sorted(ids))
    for k in range(3):
        if offset[k] > 0 and not (ids[:, k].min() < limit <= ids[:, k].max()):
            return False
        if offset[k] < 0 and not (ids[:, k].min() < -limit <= ids[:, k].max()):
            return False
    return True


@pytest.mark.parametrize("kind", ["keyframes", "degenerate"])
@pytest.mark.parametrize("pset", sc.PARAM_SETS, ids=lambda p: "v%g_t%g_r%g-%g_c%d" % p)
def test_simple_reference_oracle_and_device_arithmetic_agree_off_the_defaults(ref, oracle, pset, kind):
    host_lib = oracle_lib.load_hostcore()
    clouds0 = _clouds_of(kind, pset)
    blocks = 0
    for offset in sc.OFFSETS:
        clouds = sc.shifted(clouds0, offset)
        want = _ref_run(ref, oracle, pset, "simple", clouds)
        ora, host = _like(oracle.lib, "oracle_voxblox", pset), _like(host_lib, "hostvbx", pset)
        _integrate(ora, "simple", clouds)
        _integrate(host, "simple", clouds)
        _assert_equal(want, _blocks(ora), ("oracle", offset))
        _assert_equal(want, _blocks(host), ("hostvbx", offset))
        blocks += len(want)
    assert blocks >= 2 * len(sc.OFFSETS)


@pytest.mark.parametrize("kind", ["keyframes", "degenerate"])
@pytest.mark.parametrize("pset", sc.PARAM_SETS, ids=lambda p: "v%g_t%g_r%g-%g_c%d" % p)
def test_simple_reference_and_oracle_agree_across_voxel_index_2_23(ref, oracle, pset, kind):
    """Poses that put the scene across block id +-2^19 (voxel index +-2^23), where (float)g + 0.5 stops being exact in
    binary32: on each axis, and on all three at once.  (0.5f in oracle/tsdf_voxblox.c's voxel centre: thousands of
    distance and weight words differ here.)"""
    clouds0 = _clouds_of(kind, pset)
    for offset in sc.edge_offsets(pset[0]):
        clouds = sc.shifted(clouds0, offset)
        want = _ref_run(ref, oracle, pset, "simple", clouds)
        assert _straddles(want, offset), (offset, np.array(sorted(want)).min(0), np.array(sorted(want)).max(0))
        ora = _like(oracle.lib, "oracle_voxblox", pset)
        _integrate(ora, "simple", clouds)
        _assert_equal(want, _blocks(ora), ("oracle", offset))


# MergedTsdfIntegrator folds the points of a voxel into one, weighted by 1 / z^2 (tsdf_integrator.cc:404-416): a bundle of
# z = 0 points alone has weight 0 and a merged point of 0 / 0.  Its ray ends at voxel index (int)NaN = INT_MIN; without
# carving that is one voxel far outside any map (same in the oracle: compared), with carving the reference walks and
# allocates 2^31 voxels from the origin to it and runs out of memory.  So "merged" takes the whole degenerate cloud only
# without carving, and on every set the degenerate cloud without its weight-0 points ("weighted"); the device refuses a
# weightless bundle (tests/test_tsdf_voxblox_edges.py).
_MERGED_FAST_CASES = [(p, k, m) for p in sc.PARAM_SETS for k in ("keyframes", "degenerate", "weighted") for m in ("merged", "fast")
                      if not (m == "merged" and k == "degenerate" and p[4]) and not (m == "fast" and k == "weighted")]


@pytest.mark.parametrize("pset,kind,method", _MERGED_FAST_CASES, ids=lambda v: v if isinstance(v, str) else "v%g_t%g_r%g-%g_c%d" % v)
def test_merged_and_fast_reference_and_oracle_agree_off_the_defaults(ref, oracle, pset, kind, method):
    """MergedTsdfIntegrator and FastTsdfIntegrator (one thread, the reference's approximate sets) over the same settings
    and offsets, the edge offsets included."""
    clouds0 = _clouds_of(kind, pset)
    for offset in sc.OFFSETS + sc.edge_offsets(pset[0]):
        clouds = sc.shifted(clouds0, offset)
        want = _ref_run(ref, oracle, pset, method, clouds)
        ora = _like(oracle.lib, "oracle_voxblox", pset)
        _integrate(ora, method, clouds)
        _assert_equal(want, _blocks(ora), (method, offset))


def test_range_edge_clouds_reach_the_last_accepted_blocks_and_no_further(ref, oracle):
    """The clouds of the device's range test: blocks up to id 2^19 - 1 on +x and down to -2^19 on -y, exactly; one block
    further out they leave the accepted range.  Inside it reference == oracle == hostvbx."""
    pset = sc.PARAM_SETS[0]
    clouds = sc.range_edge_clouds(pset[0])
    want = _ref_run(ref, oracle, pset, "simple", clouds)
    ids = np.array(sorted(want))
    assert ids[:, 0].max() == sc.BLOCK_LIMIT - 1 and ids[:, 1].min() == -sc.BLOCK_LIMIT
    ora, host = _like(oracle.lib, "oracle_voxblox", pset), _like(oracle_lib.load_hostcore(), "hostvbx", pset)
    _integrate(ora, "simple", clouds)
    _integrate(host, "simple", clouds)
    _assert_equal(want, _blocks(ora), "oracle")
    _assert_equal(want, _blocks(host), "hostvbx")
    for k, c in enumerate(sc.range_edge_clouds(pset[0], shift_blocks=1)):
        far = _like(oracle.lib, "oracle_voxblox", pset)
        _integrate(far, "simple", [c])
        ids = far.chunk_ids()
        assert (ids[:, 0].max() == sc.BLOCK_LIMIT) if k == 0 else (ids[:, 1].min() == -sc.BLOCK_LIMIT - 1)


def _visit_log(host_lib, pset, cloud):
    host = _like(host_lib, "hostvbx", pset)
    f = host_lib.hostvbx_visit_log
    f.restype = ctypes.c_longlong
    f.argtypes = [_vp, _vp, _i, _vp, _vp, _vp, ctypes.c_longlong]
    xyz, _, Twc = cloud
    cap = 1 << 21
    g, ops = np.zeros((cap, 3), np.int32), np.zeros((cap, 2), np.float32)
    n = f(host.h, xyz.ctypes.data, len(xyz), np.ascontiguousarray(Twc).ctypes.data, g.ctypes.data, ops.ctypes.data, cap)
    assert 0 < n <= cap
    return g[:n], ops[:n]


_SIGNED_SETS = [sc.PARAM_SETS[0], sc.PARAM_SETS[1]] + sc.DEGENERATE_SETS[1:]


@pytest.mark.parametrize("pset", _SIGNED_SETS, ids=lambda p: "v%g_t%g_r%g-%g_c%d" % p)
def test_degenerate_cloud_feeds_the_fold_weights_that_carry_a_sign_bit(pset):
    """What the degenerate cloud is for: vb_expand marks the last record of a voxel run in the weight's sign bit, and
    updateTsdfVoxel's drop-off weight 0 * (truncation + sdf) / (truncation - voxel) of a z = 0 point can carry one itself.
    Behind the drop-off truncation + sdf < 0 (for truncation <= voxel always: sdf < -voxel), so by the sign of the
    denominator:
      truncation > voxel (the default, 0.05 / 0.2): -0.0, which std::max(uw, 0) keeps;
      truncation = voxel (0.1 / 0.1): -0.0 / 0 = NaN with the sign set;
      truncation < voxel (0.05 / 0.04, 0.2 / 0.1): negative over negative, +0.0 — these sets exercise the negative
      denominator, not the mark, and the test says so by asserting that no weight carries a sign there.
    Where there are such weights, at every offset at least 10, at least one as a voxel's only record and one inside a
    run of 16 records and more (the fold's eight-lane path); and over the offsets at least one as the LAST record of
    such a run (the log is in sequence order, the device's sort by voxel is stable)."""
    host_lib = oracle_lib.load_hostcore()
    signed = pset[1] >= pset[0]
    last_of_long = 0
    for offset in sc.DEGENERATE_OFFSETS:
        total = sole = in_long = 0
        for cloud in sc.shifted(sc.degenerate_clouds(pset[0], pset[2], pset[3]), offset):
            g, ops = _visit_log(host_lib, pset, cloud)
            uw = ops[:, 1]
            mark = np.signbit(uw) & ((uw == 0) | np.isnan(uw))
            assert not (np.signbit(uw) & ~mark).any(), "a weight is never negative"
            _, inverse, counts = np.unique(g, axis=0, return_inverse=True, return_counts=True)
            inverse = inverse.reshape(-1)
            run = counts[inverse]
            last_at = np.zeros(len(counts), np.int64)
            last_at[inverse] = np.arange(len(inverse))              # (the last assignment wins: the run's last record)
            is_last = last_at[inverse] == np.arange(len(inverse))
            total += int(mark.sum())
            sole += int((mark & (run == 1)).sum())
            in_long += int((mark & (run >= 16) & ~is_last).sum())
            last_of_long += int((mark & (run >= 16) & is_last).sum())
        if signed:
            assert total >= 10 and sole >= 1 and in_long >= 1, (offset, total, sole, in_long)
        else:
            assert total == 0, (offset, total)
    assert last_of_long >= 1 if signed else last_of_long == 0
