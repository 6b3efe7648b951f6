"""Surface extraction from the chisel map (ChunkManager::RecomputeMesh): the oracle's
properties on CPU, and the HIP path against the oracle, byte for byte, through the C ABI."""
import numpy as np
import pytest

from tests import oracle_lib
from tests.plvs_amd_synth import make_keyframes


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


def build_map(m, n_kf=4, seed=0):
    kfs = make_keyframes(n_kf, seed=seed)
    for k in kfs:
        m.integrate(k["xyz"], k["rgb"], k["kfid"], k["Twc"])
    return kfs


def test_oracle_mesh_lies_on_the_scene_surface(oracle):
    m = oracle.chisel(0.05)
    build_map(m, 3)
    ids = m.chunk_ids()
    total, on_wall = 0, 0
    for cid in ids:
        v, n, c, k = m.mesh_chunk(*cid)
        assert len(v) % 3 == 0 and len(v) == len(n) == len(c) == len(k)
        if not len(v):
            continue
        total += len(v)
        # vertices sit inside the chunk's cube of corner-to-corner cells (one voxel of slack for the border cubes)
        lo = np.array(cid, np.float32) * 0.8
        assert (v >= lo - 1e-4).all() and (v <= lo + 0.8 + 0.05 + 1e-4).all()
        ln = np.linalg.norm(n.astype(np.float64), axis=1)
        assert np.allclose(ln[ln > 0], 1.0, atol=1e-5)
        assert (c >= 0).all() and (c <= 1.0 + 1e-6).all()
        assert set(np.unique(k)) <= {0, 1, 2}
        # the room is the box |x|<=3, |y|<=2, |z|<=1.5 (plus three spheres): most vertices lie on a wall
        d = np.minimum.reduce([np.abs(np.abs(v[:, 0]) - 3.0), np.abs(np.abs(v[:, 1]) - 2.0), np.abs(np.abs(v[:, 2]) - 1.5)])
        on_wall += int((d < 0.06).sum())
    assert total > 8000 and on_wall > 0.8 * total
    # a chunk that does not exist has no mesh
    assert len(m.mesh_chunk(1000, 1000, 1000)[0]) == 0


def test_oracle_mesh_of_an_analytic_sphere(oracle):
    """The meshing restatement on a distance field with a known answer: a sphere of radius 0.55 m sampled
    into a 2 x 2 x 2 block of chunks (res 0.05).  The extracted surface must be the sphere: vertices on it,
    closed, consistently oriented (every directed edge has its reverse exactly once), genus 0, normals
    radial and pointing along the gradient, colours interpolated from the stored voxel colours."""
    res, r = 0.05, 0.55
    centre = np.array([0.8, 0.8, 0.8])
    m = oracle.chisel(res)
    idx = np.arange(16)
    for cx in range(2):
        for cy in range(2):
            for cz in range(2):
                X, Y, Z = np.meshgrid(idx + 16 * cx, idx + 16 * cy, idx + 16 * cz, indexing="ij")   # [x, y, z]
                pts = np.stack([X, Y, Z], -1) * res + res / 2
                sdf = np.linalg.norm(pts - centre, axis=-1) - r                         # > 0 outside
                # voxel id = (z * 16 + y) * 16 + x  -> array indexed [z, y, x]
                sdf_zyx = np.transpose(sdf, (2, 1, 0)).astype(np.float32)
                rgbw = np.full(4096, 200 | (100 << 8) | (50 << 16) | (254 << 24), np.uint32)
                m.set_chunk(cx, cy, cz, sdf_zyx, np.ones(4096, np.float32), np.full(4096, 9, np.uint32), rgbw)
    V, N, C, K = [], [], [], []
    for cx in range(2):
        for cy in range(2):
            for cz in range(2):
                v, n, c, k = m.mesh_chunk(cx, cy, cz)
                V.append(v); N.append(n); C.append(c); K.append(k)
    v, n, c, k = np.concatenate(V), np.concatenate(N), np.concatenate(C), np.concatenate(K)
    assert len(v) % 3 == 0 and len(v) > 3000 and (k == 9).all()
    # on the sphere (linear interpolation of a distance field: second-order error)
    d = np.linalg.norm(v.astype(np.float64) - centre, axis=1)
    assert np.abs(d - r).max() < 0.15 * res
    # closed and consistently oriented
    key = np.round(v.astype(np.float64) / (res * 1e-3)).astype(np.int64)
    _, vid = np.unique(key, axis=0, return_inverse=True)
    tri = vid.reshape(-1, 3)
    tri = tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])]     # degenerate slivers
    edges = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    fwd = {}
    for a, b in edges:
        fwd[(a, b)] = fwd.get((a, b), 0) + 1
    assert all(cnt == 1 for cnt in fwd.values()), "a directed edge is used twice: inconsistent orientation"
    assert all((b, a) in fwd for (a, b) in fwd), "the surface is not closed"
    nv, ne, nf = len(np.unique(tri)), len(fwd) // 2, len(tri)
    assert nv - ne + nf == 2, "Euler characteristic of a sphere"
    # triangle winding (p1 - p0) x (p2 - p0) and the stored gradient normal agree with the outward radial direction
    p = v.reshape(-1, 3, 3).astype(np.float64)
    geo = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    radial = p.mean(axis=1) - centre
    keep = np.linalg.norm(geo, axis=1) > 1e-9
    assert (np.einsum("ij,ij->i", geo[keep], radial[keep]) > 0).all()
    rad_v = (v - centre) / np.linalg.norm(v - centre, axis=1, keepdims=True)
    assert (np.einsum("ij,ij->i", n.astype(np.float64), rad_v) > 0.9).all()
    # colours: every voxel stores (200, 100, 50); the look-up quirk falls back to the nearest voxel -> exact
    assert np.allclose(c, np.array([200, 100, 50]) / 255.0, atol=1e-6)


def _neighbourhood(ids):
    s = set()
    for cid in ids:
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    s.add((cid[0] + dx, cid[1] + dy, cid[2] + dz))
    return sorted(s)


@pytest.mark.gpu
@pytest.mark.parametrize("res,n_kf", [(0.05, 4), (0.10, 3)])
def test_hip_mesh_matches_oracle(oracle, res, n_kf):
    from plvs_amd.tsdf import TsdfChisel
    ref, hip = oracle.chisel(res), TsdfChisel(res)
    kfs = make_keyframes(n_kf, seed=1)
    for k in kfs[:-1]:
        ref.integrate(k["xyz"], k["rgb"], k["kfid"], k["Twc"])
        hip.integrate(k["xyz"], k["rgb"], k["kfid"], k["Twc"])
    k = kfs[-1]
    ref.integrate(k["xyz"], k["rgb"], k["kfid"], k["Twc"])
    hip.integrate(k["xyz"], k["rgb"], k["kfid"], k["Twc"])
    # Chisel's meshesToUpdate: the 27-neighbourhood of the chunks the last integrate updated (Chisel.cpp:553-568);
    # it contains ids of chunks that do not exist
    todo = np.array(_neighbourhood(map(tuple, hip.updated_chunk_ids())), np.int32)
    existing = set(map(tuple, ref.chunk_ids()))
    assert any(tuple(c) not in existing for c in todo) and any(tuple(c) in existing for c in todo)
    got = hip.mesh_chunks(todo)
    first = got["chunk_first"]
    assert first[0] == 0 and first[-1] == len(got["vertices"]) > 2000
    checked = 0
    for i, cid in enumerate(todo):
        v, n, c, kf = ref.mesh_chunk(*cid)
        a, b = first[i], first[i + 1]
        assert b - a == len(v), (tuple(cid), b - a, len(v))
        if len(v):
            assert got["vertices"][a:b].tobytes() == v.tobytes()
            assert got["kfids"][a:b].tobytes() == kf.tobytes()
            assert got["colors"][a:b].tobytes() == c.tobytes()
            assert got["normals"][a:b].tobytes() == n.tobytes()
            checked += 1
    assert checked > 5
    # empty list, unknown chunks only
    e = hip.mesh_chunks(np.zeros((0, 3), np.int32))
    assert len(e["vertices"]) == 0
    e = hip.mesh_chunks(np.array([[999, 999, 999], [-999, 0, 0]], np.int32))
    assert len(e["vertices"]) == 0 and list(e["chunk_first"]) == [0, 0, 0]


@pytest.mark.gpu
def test_hip_mesh_capacity_is_reported():
    import ctypes
    from plvs_amd import _lib
    from plvs_amd.tsdf import TsdfChisel
    hip = TsdfChisel(0.05)
    build_map(hip, 2)
    ids = np.ascontiguousarray(hip.chunk_ids(), np.int32)
    first = np.zeros(len(ids) + 1, np.int32)
    n = ctypes.c_int()
    f = _lib.lib.plvs_hip_tsdf_chisel_mesh_chunks
    f.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 2
    buf = np.zeros((8, 3), np.float32)
    rc = f(hip._h, _lib.np_ptr(ids), len(ids), _lib.np_ptr(buf), _lib.np_ptr(buf.copy()), _lib.np_ptr(buf.copy()),
           _lib.np_ptr(np.zeros(8, np.uint32)), 8, _lib.np_ptr(first), ctypes.byref(n))
    assert rc == _lib.PLVS_ERR_CAPACITY and n.value > 8 and first[-1] == n.value and (buf == 0).all()


@pytest.mark.gpu
def test_hip_mesh_of_an_analytic_sphere_through_upload_chunk(oracle):
    """Chunks uploaded through the C ABI: the analytic sphere of the oracle test plus exact zeros, unobserved voxels
    and random colours / kfids, meshed on the device byte for byte as the oracle meshes it (cube configurations, flat
    edges and colour look-ups an integrated room never produces)."""
    from plvs_amd.tsdf import TsdfChisel
    res, r = 0.05, 0.55
    centre = np.array([0.8, 0.8, 0.8])
    ref, hip = oracle.chisel(res), TsdfChisel(res, max_chunks=64)
    idx = np.arange(16)
    rng = np.random.default_rng(8)
    ids = []
    for cx in range(2):
        for cy in range(2):
            for cz in range(2):
                X, Y, Z = np.meshgrid(idx + 16 * cx, idx + 16 * cy, idx + 16 * cz, indexing="ij")
                pts = np.stack([X, Y, Z], -1) * res + res / 2
                sdf = np.transpose(np.linalg.norm(pts - centre, axis=-1) - r, (2, 1, 0)).astype(np.float32).reshape(-1)
                sdf[rng.integers(0, 4096, 40)] = 0.0
                flat = rng.integers(0, 4095, 30)                                 # neighbours closer than 1e-6: the flat-edge vertex
                a = rng.uniform(1e-8, 4.9e-7, 30).astype(np.float32) * np.where(sdf[flat] < 0, -1, 1).astype(np.float32)
                sdf[flat], sdf[flat + 1] = a, -a                                 # (|s0 - s1| = 2 a < 1e-6, signs differ)
                w = np.ones(4096, np.float32)
                w[rng.integers(0, 4096, 60)] = 0.0
                kfid = rng.integers(0, 1000, 4096).astype(np.uint32)
                rgbw = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
                ref.set_chunk(cx, cy, cz, sdf, w, kfid, rgbw)
                hip.set_chunk(cx, cy, cz, sdf, w, kfid, rgbw)
                ids.append((cx, cy, cz))
    assert hip.num_chunks() == 8
    for cid in ids:                                                              # what went up comes back down
        for x, y in zip(ref.get_chunk(*cid), hip.get_chunk(*cid)):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    todo = _neighbourhood(ids)
    from tests import mesh_crafted_scenario as S
    flat_edges = sum(int(S.classes(ref, "chisel", cid)[1][256 + S.CHISEL_CLASSES.index("flat")]) for cid in ids)
    assert flat_edges > 0                                                        # the mesh holds flat-edge vertices
    m = hip.mesh_chunks(np.array(todo, np.int32))
    first, total = m["chunk_first"], 0
    for i, cid in enumerate(todo):
        v, n, c, k = ref.mesh_chunk(*cid)
        a, b = int(first[i]), int(first[i + 1])
        assert b - a == len(v), (cid, b - a, len(v))
        assert m["vertices"][a:b].tobytes() == v.tobytes() and m["normals"][a:b].tobytes() == n.tobytes(), cid
        assert m["colors"][a:b].tobytes() == c.tobytes() and m["kfids"][a:b].tobytes() == k.tobytes(), cid
        total += len(v)
    assert total > 3000
    hip.close()
