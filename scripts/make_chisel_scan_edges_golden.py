#!/usr/bin/env python3
"""Golden digests of chisel maps built by the REFERENCE'S OWN projective scan integrator for
tests/chisel_scan_edge_scenario.py (cameras with roll and pitch, edge depths, seeded voxel states, odd cameras): the
wrapper of scripts/make_chisel_scan_golden.py with one more entry point (another camera on the same map); seeded chunks go
through ref_chisel_set_chunk (oracle/ref/chisel_set_chunk_ref_wrap.cpp: DistVoxel / ColorVoxel setters).  Writes
  tests/golden/chisel_scan_edges_reference_digests.json   per stage and step: chunk count, plane digest, container-order
                                                          digest; the mesh digest at a stage's end; per stage `facts`
  tests/golden/chisel_scan_edges_reference_samples.npz    the four planes of a few chunks per stage (final map), the
                                                          uploaded chunks among them; per scan the ids of the
                                                          chunks it updated
It asserts ON THE REFERENCE'S RUN what the tests rely on, that no plane of the reference's maps holds a NaN, and that the
CPU restatement equals the reference after every step.  Dev-time tool: needs the reference tree and the compiled
reference library."""
import ctypes
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_chisel_scan_golden as G                                # noqa: E402
from tests import chisel_scan_edge_scenario as S                   # noqa: E402
from tests.chisel_scan_restatement import CLASS_COUNTERS, ScanIntegrator   # noqa: E402
from tests.test_oracle_pinned_chisel_map import RefChisel, _ptr    # noqa: E402

SAMPLE = 4
_i, _f, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p


class RefEdges(RefChisel):
    def __init__(self, wrapper, cam, res):
        super().__init__(res, cam, carving=True, carving_dist=S.CARVING_DIST, near=S.NEAR, far=S.FAR)
        self.w = ctypes.CDLL(wrapper)
        self.w.ref_chisel_scan_integrate.argtypes = [_vp] * 3 + [_i, _vp]
        self.w.ref_chisel_scan_set_camera.argtypes = [_vp] + [_f] * 4 + [_i, _i, _f, _f]

    def scan(self, f):
        c = f["cam"]
        self.w.ref_chisel_scan_set_camera(self.h, c["fx"], c["fy"], c["cx"], c["cy"], c["width"], c["height"], f["near"], f["far"])
        depth = np.ascontiguousarray(f["depth"], np.float32)
        bgr = np.ascontiguousarray(f["bgr"], np.uint8)
        Twc = np.ascontiguousarray(f["Twc"], np.float32).reshape(3, 4)
        assert depth.shape == (c["height"], c["width"]) and bgr.shape[:2] == depth.shape
        self.w.ref_chisel_scan_integrate(self.h, _ptr(depth), _ptr(bgr), bgr.shape[2], _ptr(Twc))

    def upload(self, cid, planes):
        self.set_chunk(*cid, *planes)


class RefAdapter:
    """The reference, the restatement beside it: equal after every step."""

    def __init__(self, wrapper, cam, stage):
        self.stage = stage
        self.m = RefEdges(wrapper, cam, S.RES[stage])
        self.r = ScanIntegrator(S.RES[stage], cam, S.NEAR, S.FAR, carving=True, carving_dist=S.CARVING_DIST)
        self.facts = dict(scans=0, kept=0, collected=0, integrated=0, reset=0, **{k: 0 for k in CLASS_COUNTERS})
        self.stats, self.updated = [], []

    def scan(self, f):
        before = self.m.num_chunks()
        self.m.scan(f)
        self.r.cam, self.r.near, self.r.far = f["cam"], np.float32(f["near"]), np.float32(f["far"])
        st = self.r.integrate_scan(f["depth"], f["bgr"], f["Twc"])
        assert self.m.num_chunks() - before == st["kept"], (self.stage, "kept chunks", self.m.num_chunks() - before, st["kept"])
        self.facts["scans"] += 1
        for k in self.facts:
            if k != "scans":
                self.facts[k] += st[k]
        self.stats.append(dict(listed=st["listed"], kept=st["kept"], collected=st["collected"], visits=st["visits"],
                               updated=len(st["updated"])))
        self.updated.append(np.array(sorted(st["updated"]), np.int32).reshape(-1, 3))

    def upload(self, cid, planes):
        self.m.upload(cid, planes)
        self.r.store.set(tuple(int(v) for v in cid), tuple(np.array(p) for p in planes))

    def digest(self):
        ids = self.m.chunk_ids()
        for c in ids:
            for name, a in zip(("sdf", "weight"), self.m.get_chunk(*c)[:2]):
                assert not np.isnan(a).any(), f"{self.stage}: NaN in the {name} plane of the reference's chunk {tuple(c)}"
        d = S.map_digest(ids, self.m.get_chunk)
        mine = S.map_digest(self.r.store.ids(), self.r.store.get)
        assert d == mine, f"restatement differs from the reference ({self.stage}, after {self.facts['scans']} scans): {mine} vs {d}"
        return d

    def order(self):
        return self.m.chunk_ids()

    def meshes(self):
        self.m.update_meshes()
        return S.mesh_digest(self.m.chunk_ids(), self.m.mesh_chunk)


def check_facts(f, inp):
    a = f["attitudes"]
    assert a["reset"] >= 100 and a["kept"] > 50, a
    d = f["depths"]
    for k in ("int_pos_zero", "int_neg_zero", "int_negative", "int_tiny"):     # (25.0 lies beyond the far plane's reach)
        assert d[k] >= 1, f"depths: no voxel integrated through a pixel of class {k}: {d}"
    assert d["int_pos_inf"] == 0 and d["int_neg_inf"] == 0, d
    assert d["on_pos_inf"] >= 100 and d["on_neg_inf"] >= 100 and d["on_nan"] >= 100 and d["on_negative"] >= 100, d
    v = f["voxel_states"]
    for k in ("int_cw4", "int_cw5", "int_cw255", "int_w_negative", "int_w_huge", "cand_sdf_f32_1e5_reset", "cand_sdf_above_1e5",
              "cand_sdf_below_1e5_reset", "cand_w_neg_zero", "cand_w_subnormal_reset", "cand_w_negative", "cand_w_tiny_reset"):
        assert v[k] >= 1, f"voxel_states: {k} never met: {v}"
    assert v["cand_sdf_f32_1e5_reset"] == v["cand_sdf_f32_1e5"], "float32(1e-5) is below the double 1e-5: every such voxel is reset"
    assert v["cand_sdf_above_1e5_reset"] == 0
    for stage in S.STAGES:
        assert f[stage]["integrated"] > 0 and f[stage]["collected"] > f[stage]["kept"], (stage, f[stage])


def main():
    inp = S.inputs()
    out = dict(what="sha1 digests of chisel maps built by the reference's own projective scan integrator (see "
                    "scripts/make_chisel_scan_edges_golden.py)", inputs=S.inputs_digest(inp), stages={}, facts={}, scans={})
    samples = {}
    with tempfile.TemporaryDirectory() as tmp:
        wrapper = G.build_wrapper(tmp)
        for stage in S.STAGES:
            a = RefAdapter(wrapper, inp["cam"], stage)
            out["stages"][stage] = S.run(a, stage, inp)
            out["facts"][stage] = {k: int(v) for k, v in a.facts.items()}
            out["scans"][stage] = a.stats
            ids = sorted(tuple(int(v) for v in c) for c in a.m.chunk_ids())
            first = [tuple(int(v) for v in cid) for cid, _ in inp["chunks"]] if stage == "voxel_states" else []
            rest = [c for c in ids if c not in first]
            pick = first + [rest[j] for j in np.sort(np.random.default_rng(S.SEED + 7).permutation(len(rest))[:SAMPLE])]
            planes = [a.m.get_chunk(*c) for c in pick]
            samples[stage + "_ids"] = np.array(pick, np.int32)
            for j, name in enumerate(("sdf", "weight", "kfid", "rgbw")):
                samples[f"{stage}_{name}"] = np.stack([p[j] for p in planes])
            for j, u in enumerate(a.updated):                      # the ids of the chunks each scan updated
                samples[f"{stage}_updated_{j}"] = u
            print(stage, [r["chunks"] for r in out["stages"][stage]], out["facts"][stage], flush=True)
        check_facts(out["facts"], inp)
    gdir = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gdir, "chisel_scan_edges_reference_digests.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    np.savez_compressed(os.path.join(gdir, "chisel_scan_edges_reference_samples.npz"), **samples)


if __name__ == "__main__":
    main()
