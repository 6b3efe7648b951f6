"""Marching cubes of both TSDF maps on the crafted chunks and blocks of tests/mesh_crafted_scenario.py: the conditions
of every case on the oracle alone (CPU), and the HIP kernels of tsdf_mesh.hip / tsdf_voxblox_mesh.hip against the
oracle at zero tolerance — chunk_first / block_first, vertices, normals (the triangle's, and the gradient's where
chisel writes one), colours and kfids of every entry of every mesh list.  The oracle itself is pinned on the same cases
by the compiled reference (tests/test_oracle_pinned_chisel_map.py, tests/test_oracle_pinned.py)."""
import numpy as np
import pytest

from tests import mesh_crafted_scenario as S
from tests import oracle_lib


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


@pytest.mark.parametrize("name", S.NAMES)
def test_crafted_case_reaches_what_it_is_there_for(oracle, name):
    got = S.measure(S.case(name), oracle)
    print(name, {k: (v if k != "config" else int(v[S.EMITTING].min())) for k, v in got.items()})
    S.check(name, got)


def test_class_counters_are_per_call(oracle):
    """Two calls on one chunk give the same counters (nothing accumulates between them), a chunk that does not exist
    gives zeros, and the meshes are what they were before the counting walk."""
    for name in ("single_chunk", "vbx_origin"):
        c = S.case(name)
        m = S.oracle_map(oracle, c)
        cid = c["uploads"][0][0]
        before = S.oracle_mesh(m, c["backend"], cid)
        n1, a = S.classes(m, c["backend"], cid)
        n2, b = S.classes(m, c["backend"], cid)
        assert n1 == n2 == len(before[0]) > 0 and np.array_equal(a, b) and a[:256].sum() > 0
        n0, z = S.classes(m, c["backend"], (77, 77, 77))
        assert n0 == 0 and not z.any()
        for x, y in zip(before, S.oracle_mesh(m, c["backend"], cid)):
            assert x.tobytes() == y.tobytes()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.gpu
@pytest.mark.parametrize("name", S.NAMES)
def test_hip_mesh_of_crafted_chunks_matches_oracle(oracle, name):
    from plvs_amd.tsdf import TsdfChisel, TsdfVoxblox
    c = S.case(name)
    chisel = c["backend"] == "chisel"
    ref = S.oracle_map(oracle, c)
    hip = TsdfChisel(c["res"], max_chunks=c["max_chunks"]) if chisel else TsdfVoxblox(c["res"], max_blocks=c["max_chunks"])
    for cid, *planes in c["uploads"]:
        hip.set_chunk(*cid, *planes)
    assert hip.num_chunks() == len(c["uploads"])
    for cid, *planes in c["uploads"]:                           # what went up comes down, bit for bit
        for want, got in zip(planes, hip.get_chunk(*cid)):
            assert np.array_equal(_bits(want), _bits(got)), cid
    first_key = "chunk_first" if chisel else "block_first"
    keys = ("vertices", "normals", "colors", "kfids") if chisel else ("vertices", "normals", "colors")
    mesh = lambda ids: hip.mesh_chunks(ids) if chisel else hip.mesh_blocks(ids)
    want_of = {}
    total = 0
    fresh = None                                                # the first list's mesh, from the handle that had meshed nothing
    for ids in c["lists"]:
        got = mesh(ids)
        fresh = fresh or got
        first = got[first_key]
        assert first[0] == 0 and first[-1] == len(got["vertices"])
        for i, cid in enumerate(map(tuple, ids.tolist())):
            if cid not in want_of:
                want_of[cid] = S.oracle_mesh(ref, c["backend"], cid)
            want = want_of[cid]
            a, b = int(first[i]), int(first[i + 1])
            assert b - a == len(want[0]), (cid, i, b - a, len(want[0]))         # (0 for an id that does not exist)
            for key, w in zip(keys, want):
                assert got[key][a:b].tobytes() == w.tobytes(), (name, key, cid, i)
            total += b - a
    assert total > 20000
    if name in ("lists", "vbx_lists"):
        # the scratch buffers only grow: the one-id list after the 16-id list is what the fresh handle gave for it
        # (which the loop above compared with the oracle)
        mesh(c["lists"][3])
        again = mesh(c["lists"][0])
        assert len(fresh["vertices"]) > 0
        for key in keys + (first_key,):
            assert fresh[key].tobytes() == again[key].tobytes(), key
    hip.close()
