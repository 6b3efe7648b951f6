"""Named camera poses with all three attitude angles live, for the TSDF tests (input generation only).

Every pose of tests/synth_scene.py is a yaw about world z (the office loop adds pitch, never roll), so R = [right, down,
fwd] has right_z = fwd_z = 0 and down = (0, 0, -1): no row of R^T (c - t) ever sums three non-zero products.  The poses
here look into the same room (synth_scene's 6 x 4 x 3 m box with three spheres, rendered by synth_scene._render_depth):

  yaw          a plain synth_scene pose, for comparison
  general      yaw, pitch and roll all non-zero: every |R_ij| >= 0.03 (asserted)
  steep_up, steep_down   pitch of +-70 degrees
  rolled_over  roll of 178 degrees
  axis_px, axis_ny, axis_pz, axis_nz   signed permutation matrices (looking along +x, -y, +z, -z) whose entries are exactly
               +-1 and +-0, some of the zeros negative.  axis_px's centre sits exactly on a voxel centre (that voxel gets
               pc = 0, 1 / 0, 0 * inf = NaN in u), axis_ny's exactly on a chunk face.
poses(res) -> {name: Twc [3, 4] f32}; render(Twc, cam, seed) -> depth [h, w] f32, bgr [h, w, 3] u8."""
import numpy as np

from tests.synth_scene import _render_depth

F = np.float32
ROOM = (-np.array([3.0, 2.0, 1.5]), np.array([3.0, 2.0, 1.5]))
SPHERES = [(np.array([2.3, 0.5, 0.2]), 0.4), (np.array([-2.3, -0.4, -0.3]), 0.4), (np.array([-2.0, 1.3, 0.4]), 0.4)]
AXIS_EXACT = ("axis_px", "axis_ny", "axis_pz", "axis_nz")
NAMES = ("general", "steep_up", "steep_down", "rolled_over") + AXIS_EXACT
VOXEL_CENTRE_AT = ((1, -1, 0), (3, 5, 7))      # axis_px: chunk id, voxel (x, y, z) whose centre is the camera centre
CHUNK_FACE_X = 1                               # axis_ny: the camera centre's x is the lower x face of chunks (1, ., .)


def _yaw(k):
    """synth_scene's pose k: on a circle of 1 m, looking outwards; columns right, down, fwd."""
    yaw = np.deg2rad(3.6 * k)
    pos = np.array([np.cos(yaw), np.sin(yaw), 0.1 * np.sin(2 * yaw)])
    fwd = np.array([np.cos(yaw), np.sin(yaw), 0.0])
    right = np.array([np.sin(yaw), -np.cos(yaw), 0.0])
    return np.stack([right, np.cross(fwd, right), fwd], axis=1), pos


def rodrigues(axis, angle):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def voxel_centre(chunk, voxel, res):
    """The float the integrators form for a voxel centre: (l * res + res / 2) + (id * 16) * res, all in f32."""
    res = F(res)
    return np.array([(F(v) * res + res * F(0.5)) + F(c * 16) * res for c, v in zip(chunk, voxel)], F)


def poses(res=0.05):
    out = {}

    def put(name, R, t):
        out[name] = np.ascontiguousarray(np.concatenate([np.asarray(R), np.asarray(t, np.float64)[:, None]], 1).astype(F))

    R, t = _yaw(3)
    put("yaw", R, t)
    R, t = _yaw(2)
    put("general", rodrigues((1, 2, 3), 0.9) @ R, t)
    assert np.abs(out["general"][:, :3]).min() >= F(0.03), "general: an entry of R is (nearly) zero"
    R, t = _yaw(7)                                                   # rotations about the camera's own axes
    put("steep_up", R @ rodrigues((1, 0, 0), np.deg2rad(70.0)), t)
    R, t = _yaw(11)
    put("steep_down", R @ rodrigues((1, 0, 0), np.deg2rad(-70.0)), t)
    R, t = _yaw(5)
    put("rolled_over", R @ rodrigues((0, 0, 1), np.deg2rad(178.0)), t)
    z, m = 0.0, -0.0
    exact = dict(                                                    # columns right, down, fwd; right x down = fwd
        axis_px=([[z, m, 1], [-1, z, m], [m, -1, z]], voxel_centre(*VOXEL_CENTRE_AT, res)),
        axis_ny=([[-1, z, m], [m, z, -1], [z, -1, m]], np.array([F(CHUNK_FACE_X * 16) * F(res), F(0.31), F(-0.2)], F)),
        axis_pz=([[-1, m, z], [z, -1, m], [m, z, 1]], np.array([-0.4, 0.3, -0.6], F)),
        axis_nz=([[-1, z, z], [m, 1, z], [z, m, -1]], np.array([0.5, -0.2, 0.7], F)))
    for name, (R, t) in exact.items():
        put(name, np.array(R, np.float64), t)
        Rf = out[name][:, :3]
        assert np.array_equal(np.abs(Rf).sum(0), [1, 1, 1]) and np.array_equal(np.abs(Rf).sum(1), [1, 1, 1])
        assert np.linalg.det(Rf.astype(np.float64)) == 1.0
    assert any(np.signbit(out[n][:, :3][out[n][:, :3] == 0]).any() for n in AXIS_EXACT), "no -0.0 in the exact poses"
    assert np.array_equal(out["axis_px"][:, 3], voxel_centre(*VOXEL_CENTRE_AT, res))
    return out


def render(Twc, cam, seed, noise=True):
    """The room as the pose sees it: z-depth with synth_scene's Kinect-like noise, and a random colour image."""
    Twc = np.asarray(Twc, np.float64)
    rng = np.random.default_rng(seed)
    _, _, depth = _render_depth(Twc[:, :3], Twc[:, 3], cam, ROOM, SPHERES, 1)
    if noise:
        depth = depth + rng.standard_normal(depth.shape) * (0.0012 + 0.0019 * (depth - 0.4) ** 2)
    bgr = rng.integers(0, 256, size=depth.shape + (3,), dtype=np.uint8)
    return np.ascontiguousarray(depth.astype(F)), bgr
