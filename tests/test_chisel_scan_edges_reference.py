"""The CPU restatement of the projective scan integrate (tests/chisel_scan_restatement.py) against maps THE REFERENCE
ITSELF built for tests/chisel_scan_edge_scenario.py: cameras with roll and pitch, signed-permutation poses with the
camera centre on a voxel centre and on a chunk face, +-inf / negative / -0.0 / tiny depths, voxels seeded at the edges of
the reference's comparisons, cameras whose frustum and image disagree, images smaller than a chunk's footprint.
tests/golden/chisel_scan_edges_reference_digests.json holds the reference's digests step by step and the facts of its
run, ..._samples.npz the planes of a few chunks per stage (scripts/make_chisel_scan_edges_golden.py; the compiled
reference does not exist where these tests run).  Every comparison is equality of bits or of exact counts.

What these goldens see that tests/golden/chisel_scan_reference_digests.json does not is recorded as a mutation table in
DESIGN.md §4.7: with yaw-only poses every 3-term sum of the path has a zero term, so its association order was free."""
import json
import os

import numpy as np
import pytest

from tests import camera_attitudes as A
from tests import chisel_scan_edge_scenario as S
from tests.chisel_scan_restatement import CLASS_COUNTERS, ScanIntegrator

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "chisel_scan_edges_reference_digests.json")) as f:
        g = json.load(f)
    inp = S.inputs()
    assert S.inputs_digest(inp) == g["inputs"], "the inputs changed: regenerate with scripts/make_chisel_scan_edges_golden.py"
    return g, inp, np.load(os.path.join(GOLDEN, "chisel_scan_edges_reference_samples.npz"))


def test_the_poses_are_what_they_claim():
    for res in (0.05, 0.02):
        P = A.poses(res)
        assert set(A.NAMES) | {"yaw"} == set(P)
        for name, T in P.items():
            R = T[:, :3].astype(np.float64)
            assert T.dtype == np.float32 and T.shape == (3, 4)
            assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6 and np.linalg.det(R) > 0.999, name
        assert np.abs(P["general"][:, :3]).min() >= np.float32(0.03)
        assert P["yaw"][2, 0] == 0 and P["yaw"][2, 2] == 0                       # what every other TSDF test uses
        assert abs(abs(P["steep_up"][2, 2]) - np.sin(np.deg2rad(70))) < 1e-6 and P["steep_up"][2, 2] == -P["steep_down"][2, 2]
        assert P["rolled_over"][2, 1] > 0.99                                     # the camera's down axis points up
        negative_zero = 0
        for name, fwd in zip(A.AXIS_EXACT, ((1, 0, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))):
            R = P[name][:, :3]
            assert set(np.abs(R).reshape(-1).tolist()) == {0.0, 1.0} and np.array_equal(R[:, 2], fwd), name
            negative_zero += int(np.signbit(R[R == 0]).sum())
        assert negative_zero >= 1
        assert np.array_equal(P["axis_px"][:, 3], A.voxel_centre(*A.VOXEL_CENTRE_AT, res))
        assert P["axis_ny"][0, 3] == np.float32(A.CHUNK_FACE_X * 16) * np.float32(res)


def test_the_golden_run_exercised_what_the_tests_rely_on(golden):
    g = golden[0]
    assert sorted(g["stages"]) == sorted(S.STAGES)
    f = g["facts"]
    for stage in S.STAGES:
        assert len(g["stages"][stage]) == len(S.steps(stage, golden[1])) and "mesh" in g["stages"][stage][-1]
        assert f[stage]["integrated"] > 0 and f[stage]["collected"] > f[stage]["kept"] > 8
    assert f["attitudes"]["reset"] >= 100
    d = f["depths"]
    assert min(d[k] for k in ("int_pos_zero", "int_neg_zero", "int_negative", "int_tiny")) >= 1
    assert d["int_pos_inf"] == 0 and d["int_neg_inf"] == 0
    assert min(d[k] for k in ("on_pos_inf", "on_neg_inf", "on_nan", "on_negative")) >= 100
    v = f["voxel_states"]
    assert min(v[k] for k in ("int_cw4", "int_cw5", "int_cw255", "int_w_negative", "int_w_huge", "cand_sdf_above_1e5",
                              "cand_sdf_below_1e5_reset", "cand_w_neg_zero", "cand_w_subnormal_reset", "cand_w_negative",
                              "cand_w_tiny_reset")) >= 1
    assert v["cand_sdf_f32_1e5_reset"] == v["cand_sdf_f32_1e5"] >= 1 and v["cand_sdf_above_1e5_reset"] == 0


class RestatementAdapter:
    def __init__(self, cam, stage, integrator=ScanIntegrator):
        self.r = integrator(S.RES[stage], cam, S.NEAR, S.FAR, carving=True, carving_dist=S.CARVING_DIST)
        self.facts = dict(scans=0, kept=0, collected=0, integrated=0, reset=0, **{k: 0 for k in CLASS_COUNTERS})
        self.stats, self.updated = [], []

    def scan(self, f):
        self.r.cam, self.r.near, self.r.far = f["cam"], np.float32(f["near"]), np.float32(f["far"])
        st = self.r.integrate_scan(f["depth"], f["bgr"], f["Twc"])
        self.facts["scans"] += 1
        for k in self.facts:
            if k != "scans":
                self.facts[k] += st[k]
        self.stats.append(dict(listed=st["listed"], kept=st["kept"], collected=st["collected"], visits=st["visits"],
                               updated=len(st["updated"])))
        self.updated.append(np.array(sorted(st["updated"]), np.int32).reshape(-1, 3))

    def upload(self, cid, planes):
        self.r.store.set(tuple(int(v) for v in cid), tuple(np.array(p) for p in planes))

    def digest(self):
        return S.map_digest(self.r.store.ids(), self.r.store.get)

    def order(self):
        return None

    def meshes(self):
        return {}


@pytest.fixture(scope="module")
def restated(golden):
    """Every stage through the restatement, once: {stage: (records, adapter)}."""
    out = {}
    for stage in S.STAGES:
        a = RestatementAdapter(golden[1]["cam"], stage)
        out[stage] = (S.run(a, stage, golden[1]), a)
    return out


@pytest.mark.parametrize("stage", S.STAGES)
def test_restatement_reproduces_the_reference_built_maps(golden, restated, stage):
    g, inp, samples = golden
    got, a = restated[stage]
    want = g["stages"][stage]
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert x == {k: y[k] for k in ("step", "chunks", "planes")}, f"{stage}, step {x['step']}: {x} vs {y}"
    ids = samples[stage + "_ids"]
    assert len(ids) >= 4
    if stage == "voxel_states":
        assert [tuple(int(v) for v in c) for c in ids[:2]] == [tuple(cid) for cid, _ in inp["chunks"]]
    for j, cid in enumerate(ids):
        pl = a.r.store.get(tuple(int(v) for v in cid))
        assert pl is not None, f"{stage}: chunk {cid} of the reference's map is missing"
        for k, name in enumerate(("sdf", "weight", "kfid", "rgbw")):
            assert np.array_equal(np.asarray(pl[k]).view(np.uint32), samples[f"{stage}_{name}"][j].view(np.uint32)), \
                f"{stage}: chunk {cid}, plane {name}"


@pytest.mark.parametrize("stage", S.STAGES)
def test_restatement_reproduces_the_facts_of_the_reference_run(golden, restated, stage):
    g = golden[0]
    a = restated[stage][1]
    assert a.facts == g["facts"][stage]
    assert a.stats == g["scans"][stage]
    for j, u in enumerate(a.updated):
        assert np.array_equal(u, golden[2][f"{stage}_updated_{j}"]), f"{stage}: the chunks scan {j} updated"


def test_the_voxel_at_the_camera_centre_is_left_alone(golden):
    """axis_px sits exactly on a voxel centre: pc = 0, 1 / 0 = inf, 0 * inf = NaN in u, so the voxel is not on the image —
    although the depth there would integrate it."""
    inp = golden[1]
    f = dict(inp["attitudes"][A.NAMES.index("axis_px")])
    f["depth"] = np.full_like(f["depth"], 0.0)                   # a zero depth integrates every voxel within 18 cm
    a = RestatementAdapter(inp["cam"], "attitudes")
    a.scan(f)
    chunk, (x, y, z) = A.VOXEL_CENTRE_AT
    pl = a.r.store.get(chunk)
    assert pl is not None
    i = (z * 16 + y) * 16 + x
    assert pl[1][i] == 0 and pl[0][i] == np.float32(99999.0)
    assert pl[1][i + 1] > 0 and pl[1][i + 2] > 0, "the voxels ahead of it on the optical axis (+x) were not integrated"
    assert pl[1][i - 1] == 0                                     # behind the camera
