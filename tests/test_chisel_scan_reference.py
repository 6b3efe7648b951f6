"""The projective depth + colour scan integrate (PointCloudMapChisel::InsertDepthScanColor ->
Chisel::IntegrateDepthScanColorWithOneCameraModelBGR) against maps THE REFERENCE ITSELF built:
tests/golden/chisel_scan_reference_digests.json holds, step by step, digests of what the reference's own open_chisel
sources produced for tests/chisel_scan_scenario.py (scripts/make_chisel_scan_golden.py; the compiled reference does not
exist where these tests run), tests/golden/chisel_scan_reference_samples.npz the planes of a few chunks per stage.

  * CPU: the numpy restatement (tests/chisel_scan_restatement.py) reproduces every plane digest and every sample.
    InsertCloud key frames of the `mixed` stage go through the CPU oracle, on whose map the restatement then works.  The
    steps of the `deform` stage BEHIND Chisel::Deform are not restated on the CPU: the deformed map depends on the
    reference's chunk-container order, which the CPU oracle only keeps for maps it built call by call itself; those
    steps are pinned on the GPU alone.
  * GPU: the HIP path through the C ABI reproduces every digest step by step — planes, container order (deform tracking
    on), meshes through mesh_chunks — with single calls, and the planes and meshes with the batch entry.
Every comparison is equality of bits."""
import json
import os

import numpy as np
import pytest

from tests import chisel_scan_scenario as S
from tests.chisel_scan_restatement import ScanIntegrator

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "chisel_scan_reference_digests.json")) as f:
        g = json.load(f)
    inp = S.inputs()
    assert S.inputs_digest(inp) == g["inputs"], "the synthetic inputs changed: regenerate with scripts/make_chisel_scan_golden.py"
    return g, inp, np.load(os.path.join(GOLDEN, "chisel_scan_reference_samples.npz"))


def test_the_golden_run_exercised_what_the_tests_rely_on(golden):
    g = golden[0]
    assert sorted(g["stages"]) == sorted(S.STAGES)
    for stage in S.STAGES:
        assert g["stages"][stage][-1]["chunks"] > 8
    f = g["facts"]
    assert f["plain"]["collected_gt_kept"] and f["plain"]["gated"] >= 1 and f["plain"]["zero_depth"] >= 1
    assert f["carving"]["reset"] >= 100


# ------------------------------------------------------------------ CPU: the restatement
class OracleStore:
    """An oracle chisel map behind the restatement's get / set."""

    def __init__(self, m):
        self.m = m

    def get(self, *cid):
        return self.m.get_chunk(*(cid[0] if len(cid) == 1 else cid))

    def set(self, cid, planes):
        self.m.set_chunk(*cid, *planes)

    def ids(self):
        return [tuple(int(v) for v in c) for c in self.m.chunk_ids()]


class RestatementAdapter:
    def __init__(self, cam, carving, oracle=None):
        self.o = oracle.chisel(S.RES) if oracle is not None else None
        self.r = ScanIntegrator(S.RES, cam, S.NEAR, S.FAR, carving=carving, carving_dist=S.CARVING_DIST,
                                store=OracleStore(self.o) if self.o is not None else None)

    def scan(self, depth, bgr, Twc):
        self.r.integrate_scan(depth, bgr, Twc)

    def cloud(self, kf):
        self.o.integrate(kf["xyz"], kf["rgb"], kf["kfid"], kf["Twc"])

    def digest(self):
        return S.map_digest(self.r.store.ids(), self.r.store.get)

    def order(self):
        return None

    def meshes(self):
        return {}


class StopAtDeform(Exception):
    pass


class RestatementUntilDeform(RestatementAdapter):
    def deform(self, kfids, Rt):
        raise StopAtDeform


@pytest.mark.parametrize("stage", S.STAGES)
def test_restatement_reproduces_the_reference_built_maps(golden, oracle, stage):
    g, inp, samples = golden
    want = g["stages"][stage]
    a = RestatementUntilDeform(inp["cam"], stage == "carving", oracle if stage == "mixed" else None)
    got = []
    steps = S.steps(stage, inp)
    try:
        for i, (kind, x) in enumerate(steps):
            if kind == "scan":
                a.scan(x["depth"], x["bgr"], x["Twc"])
            elif kind == "cloud":
                a.cloud(x)
            else:
                a.deform(*x)
            got.append(a.digest())
    except StopAtDeform:
        assert stage == "deform" and len(got) == 3
    assert len(got) == (len(steps) if stage != "deform" else 3)
    for i, d in enumerate(got):
        assert d == {k: want[i][k] for k in ("chunks", "planes")}, f"{stage}, step {i}: {d} vs {want[i]}"
    if stage != "deform":          # the samples are chunks of the stage's final map
        ids = samples[stage + "_ids"]
        assert len(ids) > 0
        for j, cid in enumerate(ids):
            pl = a.r.store.get(tuple(int(v) for v in cid))
            assert pl is not None, f"{stage}: chunk {cid} of the reference's map is missing"
            for k, name in enumerate(("sdf", "weight", "kfid", "rgbw")):
                assert np.array_equal(np.asarray(pl[k]).view(np.uint32), samples[f"{stage}_{name}"][j].view(np.uint32)), \
                    f"{stage}: chunk {cid}, plane {name}"


# ------------------------------------------------------------------ GPU: the HIP path through the C ABI
class DeviceAdapter:
    def __init__(self, cam, carving, track):
        from plvs_amd.tsdf import TsdfChisel
        self.cam, self.carving, self.track = cam, carving, track
        self.m = TsdfChisel(S.RES, max_chunks=1024)
        if track:
            self.m.enable_deform()

    def scan(self, depth, bgr, Twc):
        self.m.integrate_scan(depth, bgr, self.cam, Twc, near=S.NEAR, far=S.FAR, use_carving=self.carving,
                              carving_dist=S.CARVING_DIST)

    def scans(self, frames):
        import torch
        self.m.integrate_scans_dev(torch.from_numpy(np.stack([f["depth"] for f in frames])).cuda(),
                                   torch.from_numpy(np.stack([f["bgr"] for f in frames])).cuda(), self.cam,
                                   torch.from_numpy(np.stack([f["Twc"] for f in frames])).cuda(), near=S.NEAR, far=S.FAR,
                                   use_carving=self.carving, carving_dist=S.CARVING_DIST)
        torch.cuda.synchronize()

    def cloud(self, kf):
        self.m.integrate(kf["xyz"], kf["rgb"], kf["kfid"], kf["Twc"])

    def deform(self, kfids, Rt):
        assert self.m.deform(kfids, Rt)["undefined"] == 0

    def digest(self):
        return S.map_digest(self.m.chunk_ids(), self.m.get_chunk)

    def order(self):
        return self.m.chunk_order() if self.track else None

    def meshes(self):
        ids = sorted(tuple(int(v) for v in c) for c in self.m.chunk_ids())
        r = self.m.mesh_chunks(np.array(ids, np.int32))
        first = r["chunk_first"]
        per = {cid: tuple(r[k][int(first[i]):int(first[i + 1])] for k in ("vertices", "normals", "colors", "kfids"))
               for i, cid in enumerate(ids)}
        return S.mesh_digest(ids, lambda *cid: per[tuple(cid)])


@pytest.mark.gpu
@pytest.mark.parametrize("stage", S.STAGES)
def test_hip_single_calls_reproduce_the_reference_built_maps(golden, stage):
    """Scan by scan, deform tracking on: planes, the chunk container's order, and the meshes at the end."""
    g, inp, _ = golden
    a = DeviceAdapter(inp["cam"], stage == "carving", track=True)
    got = S.run(a, stage, inp)
    want = g["stages"][stage]
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert x == y, f"{stage}, step {x['step']} differs from the reference's map: {x} vs {y}"
    assert "order" in got[-1] and ("mesh" in got[-1] or stage == "deform")
    a.m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stage", [s for s in S.STAGES if s != "deform"])
def test_hip_batch_entry_reproduces_the_reference_built_maps(golden, stage):
    """Consecutive scans in ONE call of the batch entry: the planes after every such call, the meshes at the end."""
    g, inp, _ = golden
    a = DeviceAdapter(inp["cam"], stage == "carving", track=False)
    got = S.run(a, stage, inp, batch=True)
    want = {r["step"]: r for r in g["stages"][stage]}
    assert len(got) < len(want) and got[-1]["step"] == max(want)
    for x in got:
        y = {k: v for k, v in want[x["step"]].items() if k != "order"}
        assert x == y, f"{stage}, after step {x['step']} differs from the reference's map: {x} vs {y}"
    assert "mesh" in got[-1]
    a.m.close()
