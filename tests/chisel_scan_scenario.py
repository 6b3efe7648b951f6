"""One fixed sequence of projective depth + colour scans (PointCloudMapChisel::InsertDepthScanColor), run on three
implementations through thin adapters: the reference's own compiled library (scripts/make_chisel_scan_golden.py ->
tests/golden/chisel_scan_reference_digests.json), the CPU restatement and the HIP path
(tests/test_chisel_scan_reference.py).  After every step the whole map is digested as tests/chisel_golden_scenario.py
defines it.

Stages, each on a map of its own (5 cm, the quarter-size TUM1 camera, near / far plane 0.1 / 5 m):
  plain    8 consecutive scans (3.6 degrees apart), no carving
  carving  the same with carving on; in scans 4-7 a rectangle of the depth image is pushed 0.6 m further
  bgra     4 scans with a 4-channel colour image
  deform   3 scans, Chisel::Deform, 2 more scans (the chunk container's order matters)
  mixed    scans interleaved with InsertCloud key frames on one map
An adapter has scan(depth, bgr, Twc), cloud(kf), deform(kfids, Rt), digest(), order() (or None), meshes()."""
import hashlib

import numpy as np

from tests.chisel_golden_scenario import cam, map_digest, mesh_digest, motions, order_digest  # noqa: F401
from tests.synth_scene import make_keyframes, make_rgbd_frames

RES = 0.05
NEAR, FAR = 0.1, 5.0            # PointCloudMapping's minDepthDistance / maxDepthDistance (PointCloudMapChisel.cc:54-55)
CARVING_DIST = 0.05             # PointCloudMapChisel.cc:57
SEED = 211
PUSH = (slice(30, 90), slice(40, 120))   # rows, columns of the pushed rectangle
STAGES = ("plain", "carving", "bgra", "deform", "mixed")


def inputs():
    c = cam()
    frames = make_rgbd_frames(8, cam=c, seed=SEED, holes=True)
    pushed = []
    for i, f in enumerate(frames):
        d = f["depth"].copy()
        if i >= 4:
            d[PUSH] = d[PUSH] + np.float32(0.6)
        pushed.append(dict(depth=d, bgr=f["bgr"], Twc=f["Twc"]))
    rng = np.random.default_rng(SEED + 1)
    bgra = [dict(depth=f["depth"], Twc=f["Twc"],
                 bgr=np.ascontiguousarray(np.concatenate([f["bgr"], rng.integers(0, 256, f["bgr"].shape[:2] + (1,), dtype=np.uint8)], -1)))
            for f in frames[:4]]
    kfs = make_keyframes(2, cam=c, seed=SEED + 2, first=2)
    return dict(cam=c, frames=frames, pushed=pushed, bgra=bgra, kfs=kfs, Rt=motions(np.array([0]), 105, 0.03, 0.08))


def inputs_digest(inp):
    h = hashlib.sha1()
    for group in (inp["frames"], inp["pushed"], inp["bgra"]):
        for f in group:
            for name in ("depth", "bgr", "Twc"):
                h.update(np.ascontiguousarray(f[name]).tobytes())
    for k in inp["kfs"]:
        for name in ("xyz", "rgb", "kfid", "Twc"):
            h.update(np.ascontiguousarray(k[name]).tobytes())
    h.update(np.ascontiguousarray(inp["Rt"]).tobytes())
    return h.hexdigest()


def steps(stage, inp):
    """-> list of (kind, payload): 'scan' frame | 'cloud' key frame | 'deform' (kfids, Rt)"""
    if stage == "plain":
        return [("scan", f) for f in inp["frames"]]
    if stage == "carving":
        return [("scan", f) for f in inp["pushed"]]
    if stage == "bgra":
        return [("scan", f) for f in inp["bgra"]]
    if stage == "deform":
        f = inp["frames"]
        return [("scan", f[0]), ("scan", f[1]), ("scan", f[2]), ("deform", (np.array([0], np.uint32), inp["Rt"])),
                ("scan", f[3]), ("scan", f[4])]
    if stage == "mixed":
        f = inp["frames"]
        return [("scan", f[0]), ("scan", f[1]), ("cloud", inp["kfs"][0]), ("scan", f[2]), ("scan", f[3]),
                ("cloud", inp["kfs"][1]), ("scan", f[4])]
    raise KeyError(stage)


def run(a, stage, inp, batch=False):
    """-> list of per-step records.  batch: consecutive scans go to a.scans(list of frames) in one call, and a record is
    taken after each such call instead of after each scan."""
    out = []
    todo = steps(stage, inp)

    def record(i, last):
        rec = dict(step=i, **a.digest())
        order = a.order()
        if order is not None:
            rec["order"] = order_digest(order)
        if last and stage != "deform":      # (after Chisel::Deform the reference's stored meshes are moved, not rebuilt)
            rec.update(a.meshes())
        out.append(rec)

    i = 0
    while i < len(todo):
        kind, x = todo[i]
        if kind == "scan" and batch:
            j = i
            while j < len(todo) and todo[j][0] == "scan":
                j += 1
            a.scans([t[1] for t in todo[i:j]])
            i = j
        else:
            if kind == "scan":
                a.scan(x["depth"], x["bgr"], x["Twc"])
            elif kind == "cloud":
                a.cloud(x)
            else:
                a.deform(*x)
            i += 1
        record(i - 1, i == len(todo))
    return out
