"""Inputs of the voxblox edge tests (tests/test_oracle_pinned_voxblox_edges.py on the CPU, tests/test_tsdf_voxblox_edges.py
on the device): integrator settings off PointCloudMapVoxblox's defaults, poses far from the origin and at the edge of the
block range a device map accepts, and a hand-made cloud of the points a depth camera never delivers.  Pure numpy."""
import numpy as np

from tests.plvs_amd_synth import make_keyframes, TUM1

# (voxel, truncation, min_ray, max_ray, carving)
PARAM_SETS = [
    (0.05, 0.1, 0.1, 5.0, 0),      # PointCloudMapVoxblox.cc:52-71
    (0.05, 0.2, 0.1, 5.0, 1),
    (0.05, 0.04, 0.5, 3.0, 0),     # truncation below the voxel: the drop-off's denominator is negative
    (0.05, 0.15, 0.1, 2.5, 1),
    (0.2, 0.1, 0.1, 5.0, 1),       # ... and here
    (0.1, 0.1, 0.1, 5.0, 0),       # ... and zero
    (0.1, 0.1, 0.1, 5.0, 1),
    (0.03, 0.12, 1.0, 4.0, 1),
    (0.07, 0.21, 0.1, 5.0, 0),
]
DEGENERATE_SETS = [PARAM_SETS[0], PARAM_SETS[2], PARAM_SETS[6], PARAM_SETS[4]]

# added to the pose translation
OFFSETS = [
    (0.0, 0.0, 0.0),
    (0.05, 0.05, 0.05),            # the origin on a voxel corner
    (-203.3, 517.7, -88.1),
    (4096.0, -4096.0, 2048.0),
    (-30000.4, 12.2, 7.7),
]
DEGENERATE_OFFSETS = [OFFSETS[0], OFFSETS[1], OFFSETS[3]]
FAR_OFFSET = OFFSETS[2]

BLOCK_LIMIT = 1 << 19              # a device map accepts block ids in [-2^19, 2^19): voxel indices below 2^23 in magnitude


def edge_length(voxel):
    """The coordinate of the face between block 2^19 - 1 and block 2^19, as the integrator scales it (float voxel size)."""
    return float(np.float32(voxel)) * 16.0 * BLOCK_LIMIT


def edge_offsets(voxel):
    """Pose offsets that put the scene across voxel index +-2^23 on each axis, and on all three at once.  (The key frames
    look along +x from x = 1: their points lie around x = 2, and around 0 on y and z.)"""
    L = edge_length(voxel)
    return [(L - 2.0, 0.0, 0.0), (0.0, -L, 0.0), (0.0, 0.0, L), (L - 2.0, L, L), (-L - 2.0, -L, -L)]


def small_cam(scale):
    c = dict(TUM1)
    for k in ("fx", "fy", "cx", "cy"):
        c[k] = c[k] / scale
    c["width"] //= scale
    c["height"] //= scale
    return c


def _rgba(rgb):
    return np.ascontiguousarray(np.concatenate([rgb, np.full((len(rgb), 1), 255, np.uint8)], axis=1))


def shifted(clouds, offset):
    """The same clouds from poses moved by `offset` (float32 translation, as a caller would hand it over)."""
    out = []
    for xyz, rgba, Twc in clouds:
        T = np.array(Twc, np.float32).reshape(3, 4).copy()
        T[:, 3] = (T[:, 3].astype(np.float64) + np.asarray(offset, np.float64)).astype(np.float32)
        out.append((xyz, rgba, T))
    return out


_KEYFRAME_CLOUDS = None


def keyframe_clouds():
    """Two key frames of the synthetic room at an eighth of the resolution: 1200 points each."""
    global _KEYFRAME_CLOUDS
    if _KEYFRAME_CLOUDS is None:
        _KEYFRAME_CLOUDS = [(np.ascontiguousarray(k["xyz"], np.float32), _rgba(k["rgb"]),
                             np.ascontiguousarray(k["Twc"], np.float32).reshape(3, 4))
                            for k in make_keyframes(2, cam=small_cam(8), seed=11)]
        assert all(len(c[0]) == 1200 for c in _KEYFRAME_CLOUDS)
    return _KEYFRAME_CLOUDS


def _directions(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def degenerate_cloud(seed, voxel, min_ray=0.1, max_ray=5.0):
    """About 1100 camera-frame points a depth camera does not deliver: depth zero and around the 1e-6 weight threshold,
    axis-aligned rays, points on voxel corners, ray lengths on both sides of the range gates, the same point many times."""
    rng = np.random.default_rng(seed)
    parts = [_directions(rng, 300) * rng.uniform(0.3, 4.5, (300, 1))]                 # generic
    p = _directions(rng, 120) * rng.uniform(0.3, 4.5, (120, 1))                       # z = 0: weight 0
    p[:, 2] = 0.0
    parts.append(p)
    p = _directions(rng, 40) * rng.uniform(0.3, 4.5, (40, 1))                         # around getVoxelWeight's 1e-6
    p[:, 2] = np.tile(np.array([1e-6, -1e-6, 9e-7, 1.1e-6]), 10)
    parts.append(p)
    p = np.zeros((60, 3))                                                             # axis-aligned
    p[np.arange(60), rng.integers(0, 3, 60)] = rng.choice([-1.0, 1.0], 60) * rng.uniform(0.3, 4.5, 60)
    parts.append(p)
    p = _directions(rng, 80) * rng.uniform(0.3, 4.5, (80, 1))                         # on voxel corners
    parts.append(np.round(p / voxel) * voxel)
    below, above = float(np.nextafter(np.float32(0.1), np.float32(0))), float(np.nextafter(np.float32(5.0), np.float32(9)))
    for length in (0.1, 5.0, below, above, min_ray, max_ray):                          # the range gates
        parts.append(_directions(rng, 30) * length)
    rep = _directions(rng, 3) * rng.uniform(0.8, 3.0, (3, 1))                         # long voxel runs
    parts.append(np.repeat(rep, 100, axis=0))
    rep0 = _directions(rng, 3) * rng.uniform(0.8, 3.0, (3, 1))                        # ... of weight 0
    rep0[:, 2] = 0.0
    parts.append(np.repeat(rep0, 20, axis=0))
    parts.append(_directions(rng, 50) * rng.uniform(5.5, 60.0, (50, 1)))              # clearing rays
    xyz = np.ascontiguousarray(np.concatenate(parts), np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    rgba = np.ascontiguousarray(rng.integers(0, 256, (len(xyz), 4), dtype=np.uint8))
    assert np.isfinite(xyz).all()
    return xyz, rgba


_DEGENERATE = {}


def degenerate_clouds(voxel, min_ray=0.1, max_ray=5.0, weightless=True):
    """Two degenerate clouds, one from the identity pose and one from a quarter turn about z.  weightless=False leaves
    out the points of weight 0 (|z| <= 1e-6): MergedTsdfIntegrator folds a bundle of such points alone into the merged
    point 0 / 0, which the reference cannot integrate with carving and the device refuses; everything else — axis-aligned
    rays along z, voxel corners, the range gates, the repeats, the clearing rays — stays."""
    key = (voxel, min_ray, max_ray, weightless)
    if key not in _DEGENERATE:
        ident = np.eye(4, dtype=np.float32)[:3]
        turn = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0]], np.float32)
        out = []
        for seed, pose in ((5, ident), (6, turn)):
            xyz, rgba = degenerate_cloud(seed, voxel, min_ray, max_ray)
            if not weightless:
                keep = np.abs(xyz[:, 2]) > np.float32(1e-6)
                xyz, rgba = np.ascontiguousarray(xyz[keep]), np.ascontiguousarray(rgba[keep])
                assert 700 < len(xyz) < len(keep)
            out.append((xyz, rgba, pose))
        _DEGENERATE[key] = out
    return _DEGENERATE[key]


def range_edge_clouds(voxel=0.05, shift_blocks=0):
    """Two small clouds that stay inside one block each: the last block a device map accepts on +x (id 2^19 - 1) and the
    first on -y (id -2^19); shift_blocks moves both poses outwards by whole blocks."""
    rng = np.random.default_rng(17)
    block = float(np.float32(voxel)) * 16.0
    L = edge_length(voxel)
    ident = np.eye(4, dtype=np.float32)[:3]
    out = []
    for axis, sign in ((0, 1.0), (1, -1.0)):
        xyz = np.ascontiguousarray(_directions(rng, 300) * rng.uniform(0.12, 0.2, (300, 1)), np.float32)
        rgba = np.ascontiguousarray(rng.integers(0, 256, (300, 4), dtype=np.uint8))
        T = ident.copy()
        T[:, 3] = np.float32(block / 2)
        T[axis, 3] = np.float32(sign * (L - block / 2 + shift_blocks * block))
        out.append((xyz, rgba, T))
    return out
