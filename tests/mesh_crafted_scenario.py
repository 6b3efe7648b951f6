"""Crafted maps for surface extraction (ChunkManager::RecomputeMesh, MeshIntegrator::updateMeshForBlock): chunks and
blocks written voxel by voxel with set_chunk, holding what an integrated room or a sampled sphere never does — every
one of the 254 cube configurations that emit, flat edges with a sign change (the quirk vertex of either back end), edges
cut exactly in the middle, signed zeros, weights on and between the thresholds (chisel 1e-15 / 1e-12, voxblox 1e-4),
maps close enough to the origin, or coarse enough, for the eight-voxel colour blend, ids that are negative, kilometres
out and next to the id limit, and mesh lists on both sides of the scan's one-launch limit.

Pure numpy, no file is read.  Three sides use it: the oracle pinned against the compiled reference libraries
(tests/test_oracle_pinned_chisel_map.py, tests/test_oracle_pinned.py), the oracle-only condition test and the GPU test
(tests/test_tsdf_mesh_crafted.py).

A case is dict(backend, res, max_chunks, uploads=[(id, planes...)], lists=[id arrays to mesh]); planes are
(sdf, weight, kfid, rgbw) for chisel and (distance, weight, rgba) for voxblox, voxel x + 16 * (y + 16 * z) in both.

measure() walks a case on the oracle alone and returns the class counters of oracle_chisel_mesh_classes /
oracle_voxblox_mesh_classes summed over the chunks its lists mesh; check() asserts the CONDITIONS of the case on them:
what keeps a case from passing without reaching what it is there for."""
import ctypes
import functools

import numpy as np

F = np.float32
VOX = 4096
COORD_LIMIT = 1 << 20                         # chunk / block ids the device holds: [-2^20, 2^20)
VOXBLOX_COORD_LIMIT = 1 << 19                 # block ids a voxblox map accepts: [-2^19, 2^19)
SCAN_SINGLE_MAX = 49152                      # exclusive_scan_u32: one launch up to here, three beyond (12 chunks)
EMITTING = np.arange(1, 255)                  # cube configurations with at least one triangle

CHISEL_CLASSES = ("flat", "trilinear", "fallback", "color_zero", "gradient", "gradient_between", "linear_id",
                  "trilinear_linear_id")
VOXBLOX_CLASSES = ("flat", "clamp_low", "clamp_high", "unobserved")

CHISEL_WEIGHTS = ((F(0.0), 40), (F(1e-13), 40), (F(1e-15), 40), (F(1e-12), 20))
VOXBLOX_WEIGHTS = ((F(0.0), 40), (F(1e-4), 40), (np.nextafter(F(1e-4), F(1)), 40))


def block(lo, shape=(2, 2, 2)):
    return [(lo[0] + x, lo[1] + y, lo[2] + z) for z in range(shape[2]) for y in range(shape[1]) for x in range(shape[0])]


def neighbourhood(ids):
    """Chisel's meshesToUpdate of these chunks: their 27-neighbourhoods (ids of chunks that do not exist included)."""
    s = {(c[0] + dx, c[1] + dy, c[2] + dz) for c in ids for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)}
    return np.array(sorted(s), np.int32)


def _take_pairs(rng, free, n):
    """n pairs of voxels that are neighbours along x, y or z inside the chunk, none used before -> (first, second)"""
    a, b = [], []
    for i in rng.permutation(VOX):
        if len(a) == n:
            break
        axis = int(rng.integers(0, 3))
        if (int(i) >> (4 * axis)) & 15 == 15:
            continue
        j = int(i) + (1 << (4 * axis))
        if free[i] and free[j]:
            free[i] = free[j] = False
            a.append(int(i))
            b.append(j)
    assert len(a) == n
    return np.array(a), np.array(b)


def field(rng, backend):
    """One chunk / block of the random field with its crafted voxels -> planes"""
    sdf = (rng.random(VOX, dtype=F) * F(2) - F(1)) * F(0.1)
    free = np.ones(VOX, bool)
    i, j = _take_pairs(rng, free, 200)                           # flat edges with a sign change: |s0 - s1| < 1e-6
    a = rng.uniform(1e-9, 4.9e-7, 200).astype(F) * rng.choice(np.array([-1, 1], F), 200)
    sdf[i], sdf[j] = a, -a
    i, j = _take_pairs(rng, free, 200)                           # t = b / (b + b) = 0.5 exactly: the vertex on a voxel face
    b = (rng.integers(1, 64, 200).astype(F) / F(512)) * rng.choice(np.array([-1, 1], F), 200)
    sdf[i], sdf[j] = b, -b
    zeros = rng.permutation(np.flatnonzero(free))[:150]
    sdf[zeros[:100]], sdf[zeros[100:]] = F(0.0), F(-0.0)
    w = rng.uniform(0.5, 3.0, VOX).astype(F)
    at = rng.permutation(VOX)
    for value, n in (CHISEL_WEIGHTS if backend == "chisel" else VOXBLOX_WEIGHTS):
        w[at[:n]], at = value, at[n:]
    colour = rng.integers(0, 1 << 32, VOX, dtype=np.uint64).astype(np.uint32)
    if backend == "chisel":
        return sdf, w, rng.integers(0, 1 << 32, VOX, dtype=np.uint64).astype(np.uint32), colour
    return sdf, w, colour


def shell(rng):
    """A chisel chunk with no surface of its own: sdf 0.05, weight 1, random colours."""
    return (np.full(VOX, 0.05, F), np.ones(VOX, F), rng.integers(0, 1 << 32, VOX, dtype=np.uint64).astype(np.uint32),
            rng.integers(0, 1 << 32, VOX, dtype=np.uint64).astype(np.uint32))


# ------------------------------------------------------------------ the cases
def _block_case(backend, res, lo, seed, shape=(2, 2, 2), shell_ids=(), max_chunks=128):
    rng = np.random.default_rng(seed)
    ids = block(lo, shape)
    uploads = [(cid, *field(rng, backend)) for cid in ids] + [(cid, *shell(rng)) for cid in shell_ids]
    return dict(backend=backend, res=res, max_chunks=max_chunks, uploads=uploads, lists=[neighbourhood(ids)])


def _origin_5cm():
    inner = set(block((-1, -1, -1)))
    return _block_case("chisel", 0.05, (-1, -1, -1), 211, shell_ids=[c for c in block((-2, -2, -2), (4, 4, 4)) if c not in inner])


def _lists(backend, res, seed):
    """Mesh lists of 1, 12 and 13 ids (12 * 4096 counts is the scan's one-launch limit), every id twice, the ids in
    reverse, and ids of chunks that do not exist between the others."""
    c = _block_case(backend, res, (-1, -1, -1), seed)
    ids = [u[0] for u in c["uploads"]]
    missing = [(5, 5, 5), (-9, 0, 0), (0, 7, -3), (COORD_LIMIT, 0, 0), (-1, -1, 1)]
    assert not set(missing) & set(ids) and 12 * VOX == SCAN_SINGLE_MAX
    interleaved = [x for pair in zip(ids, missing + missing[:3]) for x in pair]
    c["lists"] = [np.array(l, np.int32).reshape(-1, 3) for l in
                  (ids[3:4], ids + missing[:4], ids[:4] + missing + ids[4:], [x for cid in ids for x in (cid, cid)],
                   ids[::-1], interleaved)]
    return c


LINEAR_ID_RES, LINEAR_ID_INDEX = 0.013, 26


def _linear_id():
    """The look-up that takes a linear id inside [0, 4096) for a voxel outside the chunk.  InterpolateColor reads voxel
    INDICES as metres; at res 0.013 the two roundings of 26 m disagree: floor(26 * (1 / (16 res))) is chunk 124, while
    floor((26 - 124 * 16 res) * (1 / res)) is voxel 16 of it, and the linear id names voxel (0, y + 1, z) instead.  Index 26
    lies in chunk 1, so the field is chunk (1, 1, 1).  Uniform chunks with random colours stand where the x indices
    25 .. 27 and the y and z indices 18 .. 24 send the eight look-ups, so that vertices there are coloured by the
    trilinear blend THROUGH the voxel the quirk returns: a look-up that range-checks the coordinates falls back to
    GetColorAt for them and gives other colours."""
    r = F(LINEAR_ID_RES)
    rounding, inv = F(1) / (F(16) * r), F(1) / r
    chunk_of = lambda k: int(np.floor(F(k) * rounding))
    x = chunk_of(LINEAR_ID_INDEX)
    assert int(np.floor((F(LINEAR_ID_INDEX) - F(16 * x) * r) * inv)) == 16          # the float32 arithmetic of the look-up
    along = sorted({chunk_of(k) for k in (LINEAR_ID_INDEX - 1, LINEAR_ID_INDEX, LINEAR_ID_INDEX + 1)})
    side = sorted({chunk_of(k) for k in range(18, 25)})
    return _block_case("chisel", LINEAR_ID_RES, (1, 1, 1), 277, shape=(1, 1, 1), max_chunks=256,
                       shell_ids=[(a, y, z) for a in along for y in side for z in side])


BUILDERS = {
    "origin_5cm": _origin_5cm,
    "origin_10cm": lambda: _block_case("chisel", 0.10, (-1, -1, -1), 223),
    "origin_25cm": lambda: _block_case("chisel", 0.25, (-1, -1, -1), 227),
    "res_1m": lambda: _block_case("chisel", 1.0, (-1, -1, -1), 229),
    "single_chunk": lambda: _block_case("chisel", 0.05, (3, 5, -7), 233, shape=(1, 1, 1)),
    "far": lambda: _block_case("chisel", 0.05, (4000, -4001, 2500), 239),
    "very_far": lambda: _block_case("chisel", 0.05, (100000, -100001, 70000), 241),
    "id_limit": lambda: _block_case("chisel", 0.05, (COORD_LIMIT - 2, -COORD_LIMIT, COORD_LIMIT >> 1), 251),
    "lists": lambda: _lists("chisel", 0.25, 227),
    "linear_id": _linear_id,
    "vbx_origin": lambda: _block_case("voxblox", 0.05, (-1, -1, -1), 257),
    "vbx_2cm": lambda: _block_case("voxblox", 0.02, (-1, -1, -1), 263),
    "vbx_far": lambda: _block_case("voxblox", 0.05, (4000, -4001, 2500), 269),
    "vbx_very_far": lambda: _block_case("voxblox", 0.10, (100000, -100001, 70000), 271),
    "vbx_lists": lambda: _lists("voxblox", 0.05, 257),
    # next to the id limit of a voxblox map, 168 km out at 2 cm: a float32 coordinate steps by 1.6 cm.  (The colour look-up
    # still lands on a corner of the cube that made the vertex: "unobserved" stays 0.  It leaves the cube, 2497 times on
    # the oracle, only where the step exceeds a voxel, from ids of 2^20 on, which upload_block refuses.)
    "vbx_id_limit": lambda: _block_case("voxblox", 0.02, (VOXBLOX_COORD_LIMIT - 2, -VOXBLOX_COORD_LIMIT, VOXBLOX_COORD_LIMIT >> 1), 281),
}
NAMES = tuple(BUILDERS)
CHISEL_NAMES = tuple(n for n in NAMES if not n.startswith("vbx_"))
VOXBLOX_NAMES = tuple(n for n in NAMES if n.startswith("vbx_"))
BLOCK_CASES = tuple(n for n in NAMES if n not in ("single_chunk", "linear_id", "lists", "vbx_lists"))    # the 2 x 2 x 2 cases


@functools.lru_cache(maxsize=None)
def case(name):
    """The case, built once per process.  Callers do not write into its arrays."""
    return BUILDERS[name]()


# ------------------------------------------------------------------ the oracle's side
_vp, _i = ctypes.c_void_p, ctypes.c_int


def _ptr(a):
    return a.ctypes.data_as(_vp)


def oracle_map(oracle, c):
    """The case's map on the oracle."""
    if c["backend"] == "chisel":
        m = oracle.chisel(c["res"])
        for cid, *planes in c["uploads"]:
            m.set_chunk(*cid, *planes)
        return m
    m = oracle.voxblox(c["res"])
    f = m.lib.oracle_voxblox_set_block
    f.restype, f.argtypes = None, [_vp, _i, _i, _i, _vp, _vp, _vp]
    for cid, *planes in c["uploads"]:
        f(m.h, *map(int, cid), *[_ptr(np.ascontiguousarray(p)) for p in planes])
    return m


def oracle_mesh(m, backend, cid):
    """-> the arrays the device's mesh of this chunk is compared with: chisel (vertices, normals, colors, kfids),
    voxblox (vertices, normals, colors [n, 4] u8)"""
    if backend == "chisel":
        return m.mesh_chunk(*cid)
    f = m.lib.oracle_voxblox_mesh_block
    f.restype, f.argtypes = _i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i]
    cap = VOX * 15
    v, nr, col = np.zeros((cap, 3), F), np.zeros((cap, 3), F), np.zeros((cap, 4), np.uint8)
    n = f(m.h, *map(int, cid), _ptr(v), _ptr(nr), _ptr(col), cap)
    assert n <= cap
    return v[:n].copy(), nr[:n].copy(), col[:n].copy()


def classes(m, backend, cid):
    """oracle_*_mesh_classes of one chunk -> (vertices, counters [256 + classes])"""
    names = CHISEL_CLASSES if backend == "chisel" else VOXBLOX_CLASSES
    f = getattr(m.lib, f"oracle_{backend}_mesh_classes")
    f.restype, f.argtypes = _i, [_vp, _i, _i, _i, _vp]
    out = np.zeros(256 + len(names), np.uint32)
    n = f(m.h, *map(int, cid), _ptr(out))
    return n, out


def measure(c, oracle):
    """The case on the oracle alone -> dict(vertices, config [256], one entry per class), summed over the distinct ids
    of the case's lists."""
    m = oracle_map(oracle, c)
    names = CHISEL_CLASSES if c["backend"] == "chisel" else VOXBLOX_CLASSES
    total, vertices = np.zeros(256 + len(names), np.int64), 0
    for cid in sorted({tuple(int(v) for v in x) for l in c["lists"] for x in l}):
        n, out = classes(m, c["backend"], cid)
        assert n == len(oracle_mesh(m, c["backend"], cid)[0])              # the counting walk is the meshing walk
        vertices += n
        total += out
    got = dict(vertices=vertices, config=total[:256])
    got.update({k: int(total[256 + i]) for i, k in enumerate(names)})
    # every vertex is coloured once, on one of the three paths
    assert c["backend"] != "chisel" or got["trilinear"] + got["fallback"] + got["color_zero"] == vertices
    return got


TRILINEAR_AT_LEAST = {"origin_5cm": 1, "origin_10cm": 20, "origin_25cm": 1000, "res_1m": 100000}


def check(name, got):
    """The conditions of case `name` on measure()'s counters."""
    c = case(name)
    reached = got["config"][EMITTING]
    if name in BLOCK_CASES:
        assert reached.min() >= 10, (name, int(reached.min()), EMITTING[reached < 10])
        assert got["flat"] >= 1000, (name, got["flat"])
        if c["backend"] == "chisel":
            assert got["gradient_between"] >= 1000 and got["gradient"] >= 100000, (name, got)
        else:
            assert got["clamp_high"] >= 1000, (name, got)
    elif name in ("single_chunk", "linear_id"):
        assert reached.min() >= 1 and got["flat"] >= 100, (name, int(reached.min()), got["flat"])
        # the quirk look-up must reach the colours: vertices blended through a voxel it returned.  (2 x 6 x 6 cells
        # have all eight look-ups in place; this field holds about 8 vertices a cell; a sixth of that is asked for.)
        assert name != "linear_id" or (got["linear_id"] > 0 and got["trilinear_linear_id"] >= 100), got
    else:
        assert name in ("lists", "vbx_lists")
        lens = [len(l) for l in c["lists"]]
        assert lens[:3] == [1, 12, 13] and 12 * VOX == SCAN_SINGLE_MAX < 13 * VOX, lens
        have = {u[0] for u in c["uploads"]}
        twice, rev, inter = c["lists"][3:]
        assert all(tuple(twice[2 * i]) == tuple(twice[2 * i + 1]) for i in range(8)) and len(twice) == 16
        assert [tuple(x) for x in rev] == [u[0] for u in c["uploads"]][::-1]
        assert [tuple(x) in have for x in inter] == [True, False] * 8
        assert reached.min() >= 10 and got["flat"] >= 1000, (name, got)
    if name in TRILINEAR_AT_LEAST:
        assert got["trilinear"] >= TRILINEAR_AT_LEAST[name], (name, got["trilinear"])
    if name == "single_chunk":                                   # no neighbour: every cube that leaves the chunk refuses
        assert 0 < got["config"].sum() <= 15 ** 3, int(got["config"].sum())
