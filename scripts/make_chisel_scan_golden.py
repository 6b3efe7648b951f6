#!/usr/bin/env python3
"""Golden digests of chisel maps built by the REFERENCE'S OWN projective scan integrator
(Chisel::IntegrateDepthScanColorWithOneCameraModelBGR): scripts/ref_wrap/chisel_scan_ref_wrap.cpp — calls only — is
compiled into a temporary directory against the reference's headers, oracle/ref/eigen_full and
oracle/_ref/libchisel_full_ref.so, runs tests/chisel_scan_scenario.py and writes
  tests/golden/chisel_scan_reference_digests.json   per step: chunk count, plane digest, container-order digest, and the
                                                    mesh digest at the end of a stage
  tests/golden/chisel_scan_reference_samples.npz    the four planes of a seeded sample of chunks per stage (final map)
It asserts ON THE REFERENCE'S RUN that the scenario exercises what the tests rely on, checks the CPU restatement
against the reference on the way, and times the reference's integrator on one core (profiles/chisel_scan_timing.json,
key "cpu_reference").  Dev-time tool: needs the reference tree and the compiled reference library."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import chisel_scan_scenario as S                        # noqa: E402
from tests.chisel_scan_restatement import ScanIntegrator           # noqa: E402
from tests.test_oracle_pinned_chisel_map import RefChisel, _ptr    # noqa: E402


def reference_root():
    """The reference tree: $PLVS_REFERENCE, or where oracle/ref/Makefile looks for it (its REF default)."""
    if os.environ.get("PLVS_REFERENCE"):
        return os.environ["PLVS_REFERENCE"]
    with open(os.path.join(ROOT, "oracle", "ref", "Makefile")) as f:
        for line in f:
            if line.startswith("REF") and "?=" in line:
                return line.split("?=", 1)[1].strip()
    raise SystemExit("set PLVS_REFERENCE to the reference tree")


REFERENCE = reference_root()
SAMPLE = 8                                                         # chunks per stage in the samples file


def build_wrapper(tmp, base="libchisel_full_ref.so", flags=("-O2", "-ffp-contract=off", "-fno-fast-math")):
    out = os.path.join(tmp, "scan_" + base)
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.run(["g++", *flags, "-std=c++14", "-fPIC", "-w", "-I" + os.path.join(ROOT, "oracle", "ref"),
                    "-I" + os.path.join(ROOT, "oracle", "ref", "eigen_full"),
                    "-I" + os.path.join(REFERENCE, "Thirdparty", "open_chisel", "include"), "-shared",
                    os.path.join(ROOT, "scripts", "ref_wrap", "chisel_scan_ref_wrap.cpp"), "-o", out,
                    "-L" + ref_dir, "-l:" + base, "-Wl,-rpath," + ref_dir], check=True)
    return out


class RefScan(RefChisel):
    def __init__(self, wrapper, cam, carving, res=S.RES):
        super().__init__(res, cam, carving=carving, carving_dist=S.CARVING_DIST, near=S.NEAR, far=S.FAR)
        self.scan_lib = ctypes.CDLL(wrapper)
        self.scan_lib.ref_chisel_scan_integrate.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]

    def scan(self, depth, bgr, Twc):
        depth = np.ascontiguousarray(depth, np.float32)
        bgr = np.ascontiguousarray(bgr, np.uint8)
        Twc = np.ascontiguousarray(Twc, np.float32).reshape(3, 4)
        assert depth.shape == (self.cam["height"], self.cam["width"]) and bgr.shape[:2] == depth.shape
        self.scan_lib.ref_chisel_scan_integrate(self.h, _ptr(depth), _ptr(bgr), bgr.shape[2], _ptr(Twc))


class RefAdapter:
    """The reference, with the restatement run beside it (for the list sizes of the assertions, and as a first check)."""

    def __init__(self, wrapper, cam, carving, stage):
        self.m = RefScan(wrapper, cam, carving)
        self.r = ScanIntegrator(S.RES, cam, S.NEAR, S.FAR, carving=carving, carving_dist=S.CARVING_DIST)
        self.stage, self.pure = stage, True
        self.facts = dict(kept_min=None, collected_gt_kept=True, gated=0, zero_depth=0, reset=0)

    def _planes(self):
        return {tuple(int(v) for v in c): self.m.get_chunk(*c) for c in self.m.chunk_ids()}

    def scan(self, depth, bgr, Twc):
        before = self._planes()
        self.m.scan(depth, bgr, Twc)
        after = self._planes()
        f = self.facts
        if self.pure:
            st = self.r.integrate_scan(depth, bgr, Twc)
            kept = len(after) - len(before)
            assert kept == st["kept"] and set(after) == set(self.r.store.ids()), "restatement and reference disagree on the chunks"
            f["collected_gt_kept"] &= st["collected"] > kept
            f["zero_depth"] += st["zero_depth"]
        for cid, b in before.items():
            a = after[cid]
            f["gated"] += int((((b[3] >> 24) == 5) & (a[3] == b[3]) & (a[0].view(np.uint32) != b[0].view(np.uint32))).sum())
            f["reset"] += int(((b[1] > 0) & (a[1] == 0) & (a[0] == np.float32(99999.0))).sum())

    def cloud(self, kf):
        self.pure = False
        self.m.integrate(kf["xyz"], kf["rgb"], kf["kfid"], kf["Twc"])

    def deform(self, kfids, Rt):
        self.pure = False
        self.m.deform(kfids, Rt)

    def digest(self):
        d = S.map_digest(self.m.chunk_ids(), self.m.get_chunk)
        if self.pure:
            assert d == S.map_digest(self.r.store.ids(), self.r.store.get), f"restatement differs from the reference ({self.stage})"
        return d

    def order(self):
        return self.m.chunk_ids()

    def meshes(self):
        self.m.update_meshes()
        return S.mesh_digest(self.m.chunk_ids(), self.m.mesh_chunk)


def time_reference(tmp):
    """The reference's integrator, built as the reference builds it (-O3), one core, 10 full-size scans of the office loop."""
    from tests.synth_scene import TUM1, stream_keyframe
    wrapper = build_wrapper(tmp, "libchisel_full_ref_o3.so", ("-O3", "-march=x86-64-v3"))
    import tests.test_oracle_pinned_chisel_map as T
    keep = T.REF
    T.REF = os.path.join(ROOT, "oracle", "_ref", "libchisel_full_ref_o3.so")
    try:
        m = RefScan(wrapper, dict(TUM1), False)
    finally:
        T.REF = keep
    ms = []
    for k in range(10):
        kf = stream_keyframe(k, step=1, images=True)
        t0 = time.perf_counter()
        m.scan(kf["depth_grid"], kf["rgb_grid"], kf["Twc"])
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(what="Chisel::IntegrateDepthScanColorWithOneCameraModelBGR of the reference (-O3 -march=x86-64-v3), one "
                     "core, 640 x 480 scans 0-9 of the office loop into one growing 5 cm map, wall clock per scan",
                source="scripts/make_chisel_scan_golden.py", ms_per_scan=[round(v, 2) for v in ms],
                ms_median=round(float(np.median(ms)), 2), chunks_after=m.num_chunks())


def main():
    inp = S.inputs()
    out = dict(what="sha1 digests of chisel maps built by the reference's own projective scan integrator (see "
                    "scripts/make_chisel_scan_golden.py)", inputs=S.inputs_digest(inp), resolution=S.RES, stages={}, facts={})
    samples = {}
    with tempfile.TemporaryDirectory() as tmp:
        wrapper = build_wrapper(tmp)
        for stage in S.STAGES:
            a = RefAdapter(wrapper, inp["cam"], stage == "carving", stage)
            recs = S.run(a, stage, inp)
            out["stages"][stage] = recs
            out["facts"][stage] = {k: (int(v) if not isinstance(v, bool) else v) for k, v in a.facts.items() if v is not None}
            assert recs[-1]["chunks"] > 8, (stage, recs[-1])
            ids = np.array(sorted(tuple(int(v) for v in c) for c in a.m.chunk_ids()), np.int32)
            pick = ids[np.sort(np.random.default_rng(S.SEED + 7).permutation(len(ids))[:SAMPLE])]
            planes = [a.m.get_chunk(*c) for c in pick]
            samples[stage + "_ids"] = pick
            for j, name in enumerate(("sdf", "weight", "kfid", "rgbw")):
                samples[f"{stage}_{name}"] = np.stack([p[j] for p in planes])
        f = out["facts"]
        assert f["plain"]["collected_gt_kept"], "plain: a scan kept more chunks than it collected"
        assert f["plain"]["gated"] >= 1, "plain: no voxel whose colour gate closed while its sdf went on changing"
        assert f["plain"]["zero_depth"] >= 1, "plain: no voxel integrated through a zero depth"
        assert f["carving"]["reset"] >= 100, f"carving: only {f['carving']['reset']} voxels reset"
        timing = time_reference(tmp)
    gdir = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gdir, "chisel_scan_reference_digests.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    np.savez_compressed(os.path.join(gdir, "chisel_scan_reference_samples.npz"), **samples)
    tpath = os.path.join(ROOT, "profiles", "chisel_scan_timing.json")
    doc = {}
    if os.path.exists(tpath):
        with open(tpath) as fh:
            doc = json.load(fh)
    doc["cpu_reference"] = timing
    with open(tpath, "w") as fh:
        json.dump(doc, fh, indent=1)
    print({s: [r["chunks"] for r in out["stages"][s]] for s in S.STAGES}, out["facts"], timing["ms_median"])


if __name__ == "__main__":
    main()
