"""The projective depth + colour scan integrate (Chisel::IntegrateDepthScanColorWithOneCameraModelBGR) where
tests/chisel_scan_scenario.py does not go: cameras with roll and pitch (tests/camera_attitudes.py), depth values that are
"a measurement" to the reference although no sensor means them, voxels in states at the edges of its comparisons, and
cameras the frustum and the image disagree on.  Run on the reference's own compiled library
(scripts/make_chisel_scan_edges_golden.py -> tests/golden/chisel_scan_edges_reference_*), the CPU restatement
(tests/test_chisel_scan_edges_reference.py) and the HIP path (tests/test_chisel_scan_edges.py).

Stages, each on a map of its own, carving on (quarter-size TUM1 camera, 5 cm, near / far 0.1 / 5 m unless noted):
  attitudes      one scan per pose of camera_attitudes.NAMES, then each pose again with the image centre 0.6 m further
  attitudes_2cm  general and steep_down at 2 cm, far plane 3 m
  depths         general and yaw, three scans each: patches of +inf, -inf, -0.7, -0.02, -0.0, 0, 1e-6, NaN, 25.0; the large
                 central patch is 0, -0.0, -0.02 in turn (only voxels right in front of the camera integrate through those)
  voxel_states   two chunks inside general's frustum uploaded first, seeded with a grid of sdf x weight x colour weight
                 at the edges of the reference's comparisons; then general as it is, and twice with the surface pushed back
  cameras        general through fx = fy / 2, fx = 2 fy, cx = -20, cy = height + 15, near = 0, and images of 1 x 1,
                 1 x 64 and 7 x 5 pixels
  cameras_2cm    general through fx = fy / 2 and fx = 2 fy at 2 cm, far plane 3 m: SetupFrustum takes fy twice, and only here
                 is the frustum's id box (one to two chunks of margin) tight enough for that to decide which voxels exist
A step is ('scan', frame) with frame = dict(depth, bgr, Twc, cam, near, far), or ('upload', (chunk id, four planes)).
An adapter has scan(frame), upload(cid, planes), digest(), order() (or None), meshes()."""
import hashlib

import numpy as np

from tests import camera_attitudes as A
from tests.chisel_golden_scenario import cam, map_digest, mesh_digest, order_digest  # noqa: F401
from tests.chisel_scan_restatement import SDF_EDGE, ScanIntegrator

F = np.float32
NEAR, FAR = 0.1, 5.0
CARVING_DIST = 0.05
SEED = 311
STAGES = ("attitudes", "attitudes_2cm", "depths", "voxel_states", "cameras", "cameras_2cm")
RES = dict(attitudes=0.05, attitudes_2cm=0.02, depths=0.05, voxel_states=0.05, cameras=0.05, cameras_2cm=0.02)
CENTRE = (slice(30, 90), slice(40, 120))          # rows, columns of the central rectangle (pushes, the large patch)
# border patches of the `depths` stage: (rows, columns, value)
PATCHES = ((slice(2, 22), slice(4, 34), np.inf), (slice(2, 22), slice(60, 95), -np.inf), (slice(2, 22), slice(125, 156), -0.7),
           (slice(45, 75), slice(3, 33), 1e-6), (slice(45, 75), slice(126, 158), np.nan), (slice(96, 118), slice(5, 40), 25.0),
           (slice(96, 118), slice(60, 100), np.inf), (slice(96, 118), slice(122, 157), -np.inf))
CENTRE_VALUES = (0.0, -0.0, -0.02)
SDF_VALUES = (SDF_EDGE, np.nextafter(SDF_EDGE, F(0)), np.nextafter(SDF_EDGE, F(1)), F(0), F(-0.0), F(-0.3), F(0.3), F(99999))
W_TINY = F(1e-15)
WEIGHT_VALUES = (F(0), F(-0.0), F(1e-40), W_TINY, np.nextafter(W_TINY, F(0)), np.nextafter(W_TINY, F(1)), F(-1), F(1), F(1e30))
CW_VALUES = (0, 4, 5, 255)


def frame(Twc, c, seed, near=NEAR, far=FAR):
    depth, bgr = A.render(Twc, c, seed)
    return dict(depth=depth, bgr=bgr, Twc=Twc, cam=c, near=near, far=far)


def pushed(f, by=0.6, where=CENTRE):
    d = f["depth"].copy()
    d[where] = d[where] + F(by)
    return dict(f, depth=d)


def patched(f, centre):
    d = f["depth"].copy()
    d[CENTRE] = F(centre)
    for rows, cols, v in PATCHES:
        d[rows, cols] = F(v)
    return dict(f, depth=d)


def scaled_cam(c, width, height):
    """The same field of view on a width x height image."""
    sx, sy = width / c["width"], height / c["height"]
    return dict(fx=c["fx"] * sx, fy=c["fy"] * sy, cx=c["cx"] * sx, cy=c["cy"] * sy, width=width, height=height)


def seeded_chunks(general):
    """The two chunks the `general` scan integrates most voxels of, seeded with the grid of voxel states."""
    r = ScanIntegrator(RES["voxel_states"], general["cam"], NEAR, FAR, carving=True, carving_dist=CARVING_DIST)
    r.integrate_scan(general["depth"], general["bgr"], general["Twc"])
    count = sorted(((int((r.store.get(cid)[1] > 0).sum()), cid) for cid in r.store.ids()), reverse=True)
    rng = np.random.default_rng(SEED + 5)
    grid = np.array([(i, j, k) for i in range(len(SDF_VALUES)) for j in range(len(WEIGHT_VALUES)) for k in range(len(CW_VALUES))])
    out = []
    for _, cid in count[:2]:
        g = grid[rng.permutation(4096) % len(grid)]              # every combination about 14 times, anywhere in the chunk
        sdf = np.array(SDF_VALUES, F)[g[:, 0]]
        w = np.array(WEIGHT_VALUES, F)[g[:, 1]]
        rgbw = (rng.integers(0, 1 << 24, 4096).astype(np.uint32) | (np.array(CW_VALUES, np.uint32)[g[:, 2]] << 24)).astype(np.uint32)
        out.append((cid, (sdf, w, rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32), rgbw)))
    return out


def inputs():
    c = cam()
    P5, P2 = A.poses(0.05), A.poses(0.02)
    att = [frame(P5[n], c, SEED + i) for i, n in enumerate(A.NAMES)]
    general, yaw = att[0], frame(P5["yaw"], c, SEED + 20)
    inp = dict(cam=c, names=A.NAMES)
    inp["attitudes"] = att + [pushed(f) for f in att]
    inp["attitudes_2cm"] = [frame(P2[n], c, SEED + 30 + i, far=3.0) for i, n in enumerate(("general", "steep_down"))]
    inp["depths"] = [patched(f, v) for f in (general, yaw) for v in CENTRE_VALUES]
    inp["chunks"] = seeded_chunks(general)
    whole = (slice(None), slice(None))
    inp["voxel_states"] = [general, pushed(general, 0.6, whole), pushed(general, 1.2, whole)]
    G = P5["general"]
    cams = [dict(c, fx=c["fy"] / 2), dict(c, fx=2 * c["fy"]), dict(c, cx=-20.0), dict(c, cy=c["height"] + 15.0)]
    inp["cameras"] = [frame(G, k, SEED + 40 + i) for i, k in enumerate(cams)] + [frame(G, c, SEED + 44, near=0.0)] + \
                     [frame(G, scaled_cam(c, w, h), SEED + 45 + i) for i, (w, h) in enumerate(((1, 1), (1, 64), (7, 5)))]
    inp["cameras_2cm"] = [frame(P2["general"], k, SEED + 50 + i, far=3.0) for i, k in enumerate(cams[:2])]
    return inp


def inputs_digest(inp):
    h = hashlib.sha1()
    for stage in STAGES:
        for f in inp[stage]:
            for name in ("depth", "bgr", "Twc"):
                h.update(np.ascontiguousarray(f[name]).tobytes())
            h.update(repr((sorted(f["cam"].items()), f["near"], f["far"])).encode())
    for cid, planes in inp["chunks"]:
        h.update(np.array(cid, np.int32).tobytes())
        for a in planes:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def steps(stage, inp):
    todo = [("scan", f) for f in inp[stage]]
    if stage == "voxel_states":
        todo = [("upload", ch) for ch in inp["chunks"]] + todo
    return todo


def run(a, stage, inp, batch=False):
    """-> list of per-step records.  batch: consecutive scans that share camera and planes go to a.scans(frames) in one
    call, and a record is taken after each such call."""
    out = []
    todo = steps(stage, inp)

    def record(i, last):
        rec = dict(step=i, **a.digest())
        order = a.order()
        if order is not None:
            rec["order"] = order_digest(order)
        if last:
            rec.update(a.meshes())
        out.append(rec)

    def same_call(f, g):
        return f["cam"] == g["cam"] and (f["near"], f["far"]) == (g["near"], g["far"])

    i = 0
    while i < len(todo):
        kind, x = todo[i]
        if kind == "scan" and batch:
            j = i
            while j < len(todo) and todo[j][0] == "scan" and same_call(x, todo[j][1]):
                j += 1
            a.scans([t[1] for t in todo[i:j]])
            i = j
        else:
            if kind == "scan":
                a.scan(x)
            else:
                a.upload(*x)
            i += 1
        record(i - 1, i == len(todo))
    return out
