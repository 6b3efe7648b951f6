"""The HIP projective scan integrate against maps THE REFERENCE ITSELF built for tests/chisel_scan_edge_scenario.py
(tests/golden/chisel_scan_edges_reference_*: cameras with roll and pitch, +-inf / negative / -0.0 / tiny depths, voxels
seeded at the edges of the reference's comparisons, cameras whose frustum and image disagree, images of 1 x 1 pixel):
single calls with deform tracking on, the batch entry, the stats of every call, small pools, and the refusals.  Every
comparison is equality of bits (plane, order and mesh digests) or of exact counts taken from the golden run."""
import json
import os

import numpy as np
import pytest

from tests import chisel_scan_edge_scenario as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "chisel_scan_edges_reference_digests.json")) as f:
        g = json.load(f)
    inp = S.inputs()
    assert S.inputs_digest(inp) == g["inputs"], "the inputs changed: regenerate with scripts/make_chisel_scan_edges_golden.py"
    return g, inp, np.load(os.path.join(GOLDEN, "chisel_scan_edges_reference_samples.npz"))


def id_set(ids):
    return {tuple(int(v) for v in c) for c in ids}


class DeviceAdapter:
    """calls: per call (first scan, scans, last_stats(), updated chunk ids)."""

    def __init__(self, stage, track, max_chunks=1024, alpha=False):
        from plvs_amd.tsdf import TsdfChisel
        self.m = TsdfChisel(S.RES[stage], max_chunks=max_chunks)
        self.track, self.alpha, self.calls, self.done = track, alpha, [], 0
        if track:
            self.m.enable_deform()

    def _note(self, k):
        self.calls.append((self.done, k, self.m.last_stats(), id_set(self.m.updated_chunk_ids())))
        self.done += k

    def scan(self, f):
        self.m.integrate_scan(f["depth"], f["bgr"], f["cam"], f["Twc"], near=f["near"], far=f["far"], use_carving=True,
                              carving_dist=S.CARVING_DIST)
        self._note(1)

    def scans(self, frames):
        import torch
        f = frames[0]
        bgr = np.stack([x["bgr"] for x in frames])
        if self.alpha:
            a = np.random.default_rng(5).integers(0, 256, bgr.shape[:3] + (1,), dtype=np.uint8)
            bgr = np.ascontiguousarray(np.concatenate([bgr, a], -1))
        self.m.integrate_scans_dev(torch.from_numpy(np.stack([x["depth"] for x in frames])).cuda(), torch.from_numpy(bgr).cuda(),
                                   f["cam"], torch.from_numpy(np.stack([x["Twc"] for x in frames])).cuda(), near=f["near"],
                                   far=f["far"], use_carving=True, carving_dist=S.CARVING_DIST)
        torch.cuda.synchronize()
        self._note(len(frames))

    def upload(self, cid, planes):
        self.m.set_chunk(*cid, *planes)

    def digest(self):
        return S.map_digest(self.m.chunk_ids(), self.m.get_chunk)

    def order(self):
        return self.m.chunk_order() if self.track else None

    def meshes(self):
        ids = sorted(id_set(self.m.chunk_ids()))
        r = self.m.mesh_chunks(np.array(ids, np.int32))
        first = r["chunk_first"]
        per = {cid: tuple(r[k][int(first[i]):int(first[i + 1])] for k in ("vertices", "normals", "colors", "kfids"))
               for i, cid in enumerate(ids)}
        return S.mesh_digest(ids, lambda *cid: per[tuple(cid)])


def stats_equal(a, g, samples, stage):
    """Every call's visits, new chunks and updated ids against the golden run's per-scan records."""
    per = g["scans"][stage]
    assert a.done == len(per)
    for first, k, st, updated in a.calls:
        rows = per[first:first + k]
        want = set()
        for j in range(first, first + k):
            want |= id_set(samples[f"{stage}_updated_{j}"])
        what = f"{stage}, scans {first}..{first + k - 1}"
        assert st["visits"] == sum(r["visits"] for r in rows), f"{what}: visits {st['visits']}"
        assert st["new_chunks"] == sum(r["kept"] for r in rows), f"{what}: new chunks {st['new_chunks']}"
        assert st["points"] == 0 and st["updated_chunks"] == len(want) and updated == want, f"{what}: updated chunks"


@pytest.mark.parametrize("stage", S.STAGES)
def test_hip_single_calls_reproduce_the_reference_built_maps(golden, stage):
    """Scan by scan, deform tracking on: planes, the chunk container's order, the meshes at the end, the stats."""
    g, inp, samples = golden
    a = DeviceAdapter(stage, track=True)
    got = S.run(a, stage, inp)
    want = g["stages"][stage]
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert x == y, f"{stage}, step {x['step']} differs from the reference's map: {x} vs {y}"
    assert "order" in got[-1] and "mesh" in got[-1]
    stats_equal(a, g, samples, stage)
    a.m.close()


@pytest.mark.parametrize("stage,alpha", [("attitudes", False), ("attitudes_2cm", False), ("depths", False), ("depths", True),
                                         ("voxel_states", False), ("cameras", False), ("cameras_2cm", False)])
def test_hip_batch_entry_reproduces_the_reference_built_maps(golden, stage, alpha):
    """All consecutive scans that share a camera in ONE call of the batch entry (attitudes: 16 scans whose frusta point
    in eight directions and whose id boxes differ; cameras: every call has K = 1); alpha: 4-channel colour images."""
    g, inp, samples = golden
    a = DeviceAdapter(stage, track=False, alpha=alpha)
    got = S.run(a, stage, inp, batch=True)
    want = {r["step"]: r for r in g["stages"][stage]}
    assert got[-1]["step"] == max(want)
    if stage in ("attitudes", "attitudes_2cm", "depths"):
        assert len(a.calls) == 1 and a.calls[0][1] == len(want)
    if stage == "voxel_states":
        assert [c[1] for c in a.calls] == [3]
    if stage in ("cameras", "cameras_2cm"):
        assert [c[1] for c in a.calls] == [1] * len(want)
    for x in got:
        y = {k: v for k, v in want[x["step"]].items() if k != "order"}
        assert x == y, f"{stage}, after step {x['step']} differs from the reference's map: {x} vs {y}"
    assert "mesh" in got[-1]
    stats_equal(a, g, samples, stage)
    a.m.close()


@pytest.mark.parametrize("stage", S.STAGES)
def test_a_pool_of_the_final_count_plus_8_is_enough(golden, stage):
    """What the reference creates and collects again takes no slot, whatever the attitude."""
    g, inp, _ = golden
    final = g["stages"][stage][-1]["chunks"]
    assert min(r["listed"] for r in g["scans"][stage]) > 2 * (final + 8)
    a = DeviceAdapter(stage, track=False, max_chunks=final + 8)
    got = S.run(a, stage, inp)
    assert {k: got[-1][k] for k in ("chunks", "planes")} == {k: g["stages"][stage][-1][k] for k in ("chunks", "planes")}
    a.m.close()


def test_a_full_pool_fails_the_call_and_the_map_until_it_is_cleared(golden):
    from plvs_amd import _lib
    g, inp, _ = golden
    want = g["stages"]["attitudes"]
    cap = 100
    first_over = next(i for i, r in enumerate(want) if r["chunks"] > cap)
    assert 2 <= first_over < len(inp["attitudes"]) - 1
    a = DeviceAdapter("attitudes", track=False, max_chunks=cap)
    frames = inp["attitudes"]
    for i in range(first_over):
        a.scan(frames[i])
    assert a.digest() == {k: want[first_over - 1][k] for k in ("chunks", "planes")}
    with pytest.raises(_lib.PlvsHipError) as e:
        a.scan(frames[first_over])
    assert e.value.code == _lib.PLVS_ERR_CAPACITY and "pool full" in str(e.value)
    with pytest.raises(_lib.PlvsHipError) as e:                      # poisoned: refused until clear()
        a.scan(frames[0])
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and "failed state" in str(e.value)
    with pytest.raises(_lib.PlvsHipError) as e:
        a.scans(frames[:2])
    assert e.value.code == _lib.PLVS_ERR_INVALID_ARG
    a.m.clear()
    assert a.m.num_chunks() == 0
    a.scan(frames[0])
    a.scan(frames[1])
    assert a.digest() == {k: want[1][k] for k in ("chunks", "planes")}      # what a fresh handle gives: the golden
    # the batch entry: the whole stage does not fit either
    a.m.clear()
    with pytest.raises(_lib.PlvsHipError) as e:
        a.scans(frames)
    assert e.value.code == _lib.PLVS_ERR_CAPACITY
    a.m.clear()
    a.scans(frames[:first_over])
    assert a.digest() == {k: want[first_over - 1][k] for k in ("chunks", "planes")}
    a.m.close()


def test_frusta_beyond_the_supported_extent_are_refused_and_leave_the_map_alone(golden):
    from plvs_amd import _lib
    g, inp, _ = golden
    want = g["stages"]["attitudes"]
    frames = inp["attitudes"]
    a = DeviceAdapter("attitudes", track=False)
    a.scan(frames[0])
    before = a.digest()
    assert before == {k: want[0][k] for k in ("chunks", "planes")}
    away = frames[1]["Twc"].copy()
    away[:, 3] += np.float32(1e7)
    for bad in (dict(frames[1], Twc=away), dict(frames[1], far=2000.0)):
        for call in (a.scan, lambda f: a.scans([f, f])):
            with pytest.raises(_lib.PlvsHipError) as e:
                call(bad)
            assert e.value.code == _lib.PLVS_ERR_INVALID_ARG and "frustum" in str(e.value)
            assert a.digest() == before
    a.scan(frames[1])                                           # not poisoned
    assert a.digest() == {k: want[1][k] for k in ("chunks", "planes")}
    a.m.close()
