"""Chisel::Deform on crafted chunks (tests/deform_crafted_scenario.py): long claimant runs and the colour freeze, the
"known" threshold, kfids beyond 2^31, the sort's path switches, chunk ids next to +-2^20, a pool met exactly, empty
outcomes, refusals and non-finite transformations.  The oracle (pinned on the same cases against the compiled reference
library in tests/test_oracle_pinned_chisel_map.py) must reach every case's conditions on the CPU; the device must equal
the oracle — container order, every voxel bit for bit, the counters and the meshes — after every step."""
import ctypes

import numpy as np
import pytest

from tests import deform_crafted_scenario as S
from tests import oracle_lib
from tests.test_tsdf_chisel import compare_maps
from tests.test_tsdf_deform import order_of
from tests.test_tsdf_mesh import _neighbourhood


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib.load()


SCALARS = ("new_chunks", "moved", "discarded", "undefined", "known_before", "chunks_before", "longest_run", "new_voxels",
           "shared", "at_cw254", "freeze_discards")


@pytest.mark.parametrize("name", S.NAMES)
def test_oracle_reaches_the_conditions_of_the_case(oracle, name):
    c = S.case(name)
    got = S.measure(oracle, c)
    for tag, g in got.items():
        print(name, tag, {k: g[k] for k in SCALARS if k in g}, "refused" if g["refused"] else "")
    S.check(name, c, got)


# ------------------------------------------------------------------ GPU
def snapshot(dev):
    ids = sorted(tuple(int(v) for v in c) for c in dev.chunk_ids())
    return ids, order_of(dev), [tuple(p.tobytes() for p in dev.get_chunk(*cid)) for cid in ids]


def agree(ora, dev):
    assert order_of(dev) == order_of(ora)
    return compare_maps(ora, dev, tol=0.0)


def meshes_agree(ora, dev):
    """mesh_chunks over the 27-neighbourhood of every chunk of the map == the oracle's mesh_chunk, byte for byte."""
    todo = np.array(_neighbourhood(map(tuple, dev.chunk_ids().tolist())), np.int32)
    got = dev.mesh_chunks(todo)
    first = got["chunk_first"]
    assert first[0] == 0 and first[-1] == len(got["vertices"])
    for i, cid in enumerate(todo):
        v, n, col, kf = ora.mesh_chunk(*cid)
        a, b = first[i], first[i + 1]
        assert b - a == len(v), (tuple(cid), b - a, len(v))
        for name, x, y in zip(("vertices", "normals", "colors", "kfids"), (v, n, col, kf),
                              (got["vertices"], got["normals"], got["colors"], got["kfids"])):
            assert y[a:b].tobytes() == x.tobytes(), (name, tuple(cid))
    return len(got["vertices"])


def both_integrate(ora, dev, kf):
    ora.integrate(kf["xyz"], kf["rgb"], kf["kfid"], kf["Twc"])
    ora.end_call()
    dev.integrate(kf["xyz"], kf["rgb"], kf["kfid"], kf["Twc"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", S.NAMES)
def test_hip_deform_of_crafted_chunks_equals_the_oracle(oracle, name):
    from plvs_amd import _lib
    from plvs_amd.tsdf import TsdfChisel
    c = S.case(name)
    ora = oracle.chisel(c["res"]).track_order()
    dev = TsdfChisel(c["res"], max_chunks=c["max_chunks"]).enable_deform()
    deforms = refusals = 0
    for step in c["steps"]:
        if step[0] == "upload":
            for cid, *planes in step[1]:
                ora.set_chunk(*cid, *planes)
                dev.set_chunk(*cid, *planes)
            agree(ora, dev)
        elif step[0] == "integrate":
            both_integrate(ora, dev, step[1])
            agree(ora, dev)
        elif step[0] == "mesh":
            assert meshes_agree(ora, dev) > 0
        elif step[0] == "refuse":
            before = snapshot(dev)
            with pytest.raises(_lib.PlvsHipError) as e:
                dev.deform(step[2], step[3])
            assert e.value.code == _lib.PLVS_ERR_CAPACITY
            assert snapshot(dev) == before
            agree(ora, dev)
            refusals += 1
        else:
            moving = S.walk(ora, c["res"], step[2], step[3])["moved"]
            want = ora.deform(step[2], step[3])
            got = dev.deform(step[2], step[3])
            assert want[2] == 0
            assert (got["new_chunks"], got["discarded"], got["undefined"]) == want and got["moved"] == moving, (step[1], got, want, moving)
            assert agree(ora, dev) == want[0]
            assert len(dev.updated_chunk_ids()) == 0
            deforms += 1
    assert deforms == sum(s[0] == "deform" for s in c["steps"]) > 0
    assert refusals == sum(s[0] == "refuse" for s in c["steps"])
    dev.close()


def _bad_maps():
    good = S.small_motions(2, np.random.default_rng(5))
    out = {}
    for name, at, value in (("nan_in_R", 12 + 4, np.nan), ("nan_in_t", 12 + 10, np.nan), ("inf_in_t", 11, np.inf)):
        Rt = good.copy()
        Rt.reshape(-1)[at] = value
        out[name] = Rt
    return good, out


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["nan_in_R", "nan_in_t", "inf_in_t"])
def test_hip_deform_refuses_a_transformation_that_is_not_finite(oracle, which):
    """(int)floorf(NaN) is 0 on the device and INT_MIN in the reference, which then indexes out of bounds: there is nothing
    to be equal to, so the call is refused with the map (and the mesh) untouched."""
    from plvs_amd import _lib
    from plvs_amd.tsdf import TsdfChisel
    c = S.case("thresholds")
    good, bad = _bad_maps()
    kfids = np.array([0, 1], np.uint32)
    ora = oracle.chisel(c["res"]).track_order()
    dev = TsdfChisel(c["res"], max_chunks=c["max_chunks"]).enable_deform()
    for cid, *planes in c["steps"][0][1]:
        ora.set_chunk(*cid, *planes)
        dev.set_chunk(*cid, *planes)
    before = snapshot(dev)
    with pytest.raises(_lib.PlvsHipError) as e:
        dev.deform(kfids, bad[which])
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG
    assert snapshot(dev) == before
    # the mesh half, through the C entry point: it works in place on the caller's arrays
    rng = np.random.default_rng(7)
    v, nr = rng.normal(size=(300, 3)).astype(np.float32), rng.normal(size=(300, 3)).astype(np.float32)
    vk = rng.integers(0, 3, 300).astype(np.uint32)
    v0, n0 = v.copy(), nr.copy()
    f = _lib.lib.plvs_hip_tsdf_chisel_deform_mesh
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int]
    assert f(_lib.np_ptr(v), _lib.np_ptr(nr), _lib.np_ptr(vk), 300, _lib.np_ptr(kfids), _lib.np_ptr(bad[which]), 2) == _lib.PLVS_ERR_INVALID_ARG
    assert v.tobytes() == v0.tobytes() and nr.tobytes() == n0.tobytes()
    assert f(_lib.np_ptr(v), _lib.np_ptr(nr), _lib.np_ptr(vk), 300, _lib.np_ptr(kfids), _lib.np_ptr(good), 2) == _lib.PLVS_OK
    want_v, want_n = ora.deform_mesh(v0, n0, vk, kfids, good)
    assert v.tobytes() == want_v.tobytes() and nr.tobytes() == want_n.tobytes()
    # the device-pointer form reads a table it can read: pinned host memory (refused before any launch)
    import torch
    g = _lib.lib.plvs_hip_tsdf_chisel_deform_mesh_dev
    g.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p]
    pinned = [torch.from_numpy(a.view(np.int32).reshape(-1).copy()).pin_memory() for a in (v0, n0, vk, kfids, bad[which])]
    assert g(*[_lib.t_ptr(t) for t in pinned[:3]], 300, *[_lib.t_ptr(t) for t in pinned[3:]], 2, None) == _lib.PLVS_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert pinned[0].numpy().tobytes() == v0.tobytes() and pinned[1].numpy().tobytes() == n0.tobytes()
    # the handle is as usable as before
    want = ora.deform(kfids, good)
    got = dev.deform(kfids, good)
    assert (got["new_chunks"], got["discarded"], got["undefined"]) == want
    agree(ora, dev)
    dev.close()


def _mesh_inputs(n, seed):
    rng = np.random.default_rng(seed)
    v = (rng.normal(size=(n, 3)) * 3).astype(np.float32)
    nr = rng.normal(size=(n, 3)).astype(np.float32)
    return v, nr, rng


def _mesh_variants(n):
    """-> [(label, vertices, normals, vertex kfids, kfids, Rt)]"""
    big = next(s for s in S.case("kfid_map")["steps"] if s[0] == "deform" and s[1] == "a")
    out = []
    v, nr, rng = _mesh_inputs(n, 11 + n)
    out.append(("no_map", v, nr, rng.integers(0, 4, n).astype(np.uint32), np.zeros(0, np.uint32), np.zeros((0, 12), np.float32)))
    out.append(("one_entry", v, nr, rng.integers(6, 9, n).astype(np.uint32), np.array([7], np.uint32), S.small_motions(1, rng, rot=0.4)))
    # kfids beyond 2^31 in a map of 5000 entries; 1, 2^31 - 1, 2^32 - 2 and 12345 have no entry: those vertices stay
    out.append(("wide_kfids", v, nr, rng.choice(np.array(S.VOXEL_KFIDS, np.uint32), n), big[2], big[3]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 257, 10007])
def test_hip_deform_mesh_equals_the_oracle(oracle, n):
    import torch
    from plvs_amd import _lib
    from plvs_amd.tsdf import TsdfChisel
    ora = oracle.chisel(0.05)
    f = _lib.lib.plvs_hip_tsdf_chisel_deform_mesh_dev
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p]
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1)).cuda()
    for label, v, nr, vk, kfids, Rt in _mesh_variants(n):
        want_v, want_n = ora.deform_mesh(v, nr, vk, kfids, Rt)
        hit = np.isin(vk, kfids)
        assert np.array_equal(want_v[~hit], v[~hit]) and np.array_equal(want_n[~hit], nr[~hit])
        if n >= 255 and len(kfids):
            assert 0 < hit.sum() < n and (want_v[hit] != v[hit]).any(), label      # vertices with and without an entry
        got_v, got_n = TsdfChisel.deform_mesh(v, nr, vk, kfids, Rt)
        assert got_v.tobytes() == want_v.tobytes() and got_n.tobytes() == want_n.tobytes(), label
        d = [up(a) for a in (v, nr, vk, kfids, Rt)]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            rc = f(*[_lib.t_ptr(t) if t.numel() else None for t in d[:3]], n,
                   *[_lib.t_ptr(t) if t.numel() else None for t in d[3:]], len(kfids), ctypes.c_void_p(stream.cuda_stream))
        assert rc == _lib.PLVS_OK, label
        stream.synchronize()
        assert d[0].cpu().numpy().tobytes() == want_v.tobytes() and d[1].cpu().numpy().tobytes() == want_n.tobytes(), label
