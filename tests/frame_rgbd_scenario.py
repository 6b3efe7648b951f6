"""Seeded scenario behind tests/golden/frame_rgbd_reference.npz: a 64 x 48 depth image stored with a pitch of 80 floats, a
calibration, ~500 key points and ~400 lines (distorted / undistorted twins a fraction of a pixel apart) for
Frame::ComputeStereoFromRGBD and Frame::ComputeStereoLinesFromRGBD.  The scene: a slanted plane, a foreground box, a patch
0.12 m from the camera (short 3-D lines), a ramp along the viewing direction (view-angle rejections), a 6 x 6 hole (lines
without a valid middle) and 9 % zero / NaN / +inf / negative pixels.  scripts/make_frame_rgbd_golden.py runs the reference
on it and asserts, on that run, that every branch is taken (tests/golden/frame_rgbd_reference_facts.json)."""
import hashlib

import numpy as np

SEED = 20240611
W, H, PITCH = 64, 48, 80
K4 = np.array([52.5, 52.25, 31.75, 23.5], np.float32)        # fx, fy, cx, cy
MBF = np.float32(4.0)
MIN_LINE_LENGTH_3D = np.float32(0.01)
N_POINTS, N_RANDOM_LINES, N_HOLE_LINES, N_NEAR_LINES = 500, 384, 10, 6
HOLE = (40, 8, 6)              # x0, y0, side
NEAR = (44, 30, 12)            # the 0.12 m patch
PAD = np.float32(-7.0)         # what lies between width and pitch: never to be read

KP_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32), ("response", np.float32),
                     ("octave", np.int32), ("class_id", np.int32)])
KEYLINE_DTYPE = np.dtype([("angle", np.float32), ("class_id", np.int32), ("octave", np.int32), ("pt_x", np.float32),
                          ("pt_y", np.float32), ("response", np.float32), ("size", np.float32),
                          ("startPointX", np.float32), ("startPointY", np.float32), ("endPointX", np.float32),
                          ("endPointY", np.float32), ("sPointInOctaveX", np.float32), ("sPointInOctaveY", np.float32),
                          ("ePointInOctaveX", np.float32), ("ePointInOctaveY", np.float32),
                          ("lineLength", np.float32), ("numOfPixels", np.int32)])


def _scene(rng):
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    d = (np.float32(2.0) + np.float32(0.01) * x + np.float32(0.015) * y).astype(np.float32)      # slanted plane
    d[12:28, 18:36] = np.float32(1.0) + np.float32(0.002) * x[12:28, 18:36]                      # foreground box
    nx, ny, ns = NEAR
    d[ny:ny + ns, nx:nx + ns] = np.float32(0.12)                                                 # near patch
    d[30:46, 4:20] = np.float32(1.0) + np.float32(0.06) * (x[30:46, 4:20] - np.float32(4))       # ramp along the view
    bad = rng.random((H, W)) < 0.09
    kind = rng.integers(0, 4, (H, W))
    d[bad & (kind == 0)] = 0.0
    d[bad & (kind == 1)] = np.nan
    d[bad & (kind == 2)] = np.inf
    d[bad & (kind == 3)] = -1.5
    hx, hy, hs = HOLE
    d[hy:hy + hs, hx:hx + hs] = 0.0                                                              # the hole
    return d


def _directions(rng, n):
    """Unit vectors from +, *, / and sqrt alone (correctly rounded everywhere: the inputs digest holds on every machine)."""
    d = rng.uniform(-1.0, 1.0, (n, 2))
    return d / np.sqrt(np.maximum(d[:, :1] * d[:, :1] + d[:, 1:] * d[:, 1:], 1e-6))


def _keylines(seg):
    kl = np.zeros(len(seg), KEYLINE_DTYPE)
    kl["startPointX"], kl["startPointY"], kl["endPointX"], kl["endPointY"] = seg.T
    kl["sPointInOctaveX"], kl["sPointInOctaveY"], kl["ePointInOctaveX"], kl["ePointInOctaveY"] = seg.T
    kl["pt_x"], kl["pt_y"] = (seg[:, 0] + seg[:, 2]) / 2, (seg[:, 1] + seg[:, 3]) / 2
    kl["lineLength"] = np.sqrt((seg[:, 2] - seg[:, 0]) ** 2 + (seg[:, 3] - seg[:, 1]) ** 2)
    kl["class_id"] = np.arange(len(seg))
    return kl


def inputs():
    rng = np.random.default_rng(SEED)
    image = _scene(rng)
    pitched = np.full((H, PITCH), PAD, np.float32)
    pitched[:, :W] = image
    # key points: anywhere inside the image, the last 24 on the last column / the last row
    xy = np.stack([rng.uniform(0, W, N_POINTS), rng.uniform(0, H, N_POINTS)], -1).astype(np.float32)
    xy[-24:-12, 0] = np.float32(W - 1) + rng.uniform(0, 0.99, 12).astype(np.float32)
    xy[-12:, 1] = np.float32(H - 1) + rng.uniform(0, 0.99, 12).astype(np.float32)
    kps = np.zeros(N_POINTS, KP_DTYPE)
    kps["x"], kps["y"] = xy[:, 0], xy[:, 1]
    kps["size"], kps["angle"], kps["class_id"] = 31.0, rng.uniform(0, 360, N_POINTS), -1
    kps_un = kps.copy()
    kps_un["x"] += rng.uniform(-0.4, 0.4, N_POINTS).astype(np.float32)
    kps_un["y"] += rng.uniform(-0.4, 0.4, N_POINTS).astype(np.float32)
    # lines: end points in [-1, W] x [-1, H]; a quarter of the random ones 1.5 - 3.5 px long
    lo, hi = np.array([-1, -1], np.float32), np.array([W, H], np.float32)
    s = rng.uniform(lo, hi, (N_RANDOM_LINES, 2))
    e = rng.uniform(lo, hi, (N_RANDOM_LINES, 2))
    short = np.arange(N_RANDOM_LINES) % 4 == 3
    e[short] = np.clip(s[short] + (rng.uniform(1.5, 3.5, (N_RANDOM_LINES, 1)) * _directions(rng, N_RANDOM_LINES))[short], lo, hi)
    # ... placed on purpose: lines whose middle lies inside the hole (no valid middle), short lines on the near patch
    hx, hy, hs = HOLE
    mid = np.array([hx + hs / 2, hy + hs / 2]) + rng.uniform(-0.9, 0.9, (N_HOLE_LINES, 2))
    half = np.stack([rng.uniform(5.5, 9.0, N_HOLE_LINES), rng.uniform(-2.0, 2.0, N_HOLE_LINES)], -1)
    nx, ny, ns = NEAR
    ns_ = np.array([nx + 3, ny + 3]) + rng.uniform(0, ns - 6, (N_NEAR_LINES, 2))
    ne = ns_ + rng.uniform(1.5, 2.5, (N_NEAR_LINES, 1)) * _directions(rng, N_NEAR_LINES)
    seg = np.concatenate([np.concatenate([s, e], -1), np.concatenate([mid - half, mid + half], -1),
                          np.concatenate([ns_, ne], -1)]).astype(np.float32)
    seg = seg[rng.permutation(len(seg))]
    seg_un = (seg + rng.uniform(-0.4, 0.4, seg.shape)).astype(np.float32)
    return dict(depth=pitched, width=W, height=H, pitch=PITCH, K4=K4.copy(), mbf=MBF, min_line_length_3d=MIN_LINE_LENGTH_3D,
                kps=kps, kps_un=kps_un, keylines=_keylines(seg), keylines_un=_keylines(seg_un))


def image_of(inp):
    """The height x width view of the pitched image."""
    return inp["depth"][:, :inp["width"]]


def lines8(inp):
    """Per line: uS vS uE vE of the distorted line, then of the undistorted one (what the restatement reads)."""
    f = ("startPointX", "startPointY", "endPointX", "endPointY")
    return np.stack([inp["keylines"][k] for k in f] + [inp["keylines_un"][k] for k in f], -1)


def inputs_digest(inp):
    h = hashlib.sha1()
    for k in ("depth", "K4", "kps", "kps_un", "keylines", "keylines_un"):
        h.update(np.ascontiguousarray(inp[k]).tobytes())
    h.update(np.float32(inp["mbf"]).tobytes() + np.float32(inp["min_line_length_3d"]).tobytes())
    return h.hexdigest()


def timing_inputs(n_points=2000, n_lines=100, width=640, height=480):
    """The measured workload (profiles/frame_rgbd_timing.json): a 640 x 480 plane-and-box depth image with holes and NaN, 2000
    key points and 100 lines of 20 - 120 px.  Not pinned by a golden file: timing only."""
    rng = np.random.default_rng(SEED + 1)
    x, y = np.meshgrid(np.arange(width, dtype=np.float32), np.arange(height, dtype=np.float32))
    d = (np.float32(1.5) + np.float32(0.002) * x + np.float32(0.001) * y).astype(np.float32)
    d[160:320, 200:440] = np.float32(0.9)
    bad = rng.random((height, width)) < 0.05
    d[bad] = np.where(rng.random(int(bad.sum())) < 0.5, np.float32(0), np.float32(np.nan))
    kps = np.zeros(n_points, KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, width, n_points), rng.uniform(0, height, n_points)
    s = rng.uniform([0, 0], [width, height], (n_lines, 2))
    e = np.clip(s + rng.uniform(20, 120, (n_lines, 1)) * _directions(rng, n_lines), [0, 0], [width - 1, height - 1])
    seg = np.concatenate([s, e], -1).astype(np.float32)
    return dict(depth=d, width=width, height=height, pitch=width, K4=np.array([525.0, 525.0, 319.5, 239.5], np.float32),
                mbf=np.float32(40.0), min_line_length_3d=MIN_LINE_LENGTH_3D, kps=kps, kps_un=kps.copy(), keylines=_keylines(seg),
                keylines_un=_keylines(seg))
