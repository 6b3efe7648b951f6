"""Crafted maps for Chisel::Deform (ChunkManager.cpp:918-1063): chunks written voxel by voxel with set_chunk, and
deformation maps that reach what room scans under small rigid motions never do — runs of thousands of claimants in one
new voxel, the colour freeze at weight 254, weights on both sides of the 1e-15 "known" threshold, kfids beyond 2^31,
record counts at the sort's path switches, chunk ids next to +-2^20, a pool met exactly, and the empty outcomes.

Pure numpy, no file is read.  Three sides use it: the oracle pinned against the compiled reference library
(tests/test_oracle_pinned_chisel_map.py), the oracle-only condition test and the GPU test
(tests/test_tsdf_deform_crafted.py).

A case is dict(res, max_chunks, steps); a step is one of
    ("upload", [(chunk id, sdf, weight, kfid, rgbw), ...])   set_chunk in this order
    ("integrate", key frame)                                 one cloud (tests/synth_scene.make_keyframes)
    ("deform", tag, kfids, Rt)                               Rt [n, 12]: R row-major, then t
    ("refuse", tag, kfids, Rt)                               a deform the device must refuse; the oracle's map stays
    ("mesh",)                                                the 27-neighbourhood of every chunk of the map is meshed

measure() walks a case on the oracle alone and returns, per tag, the class counters of that deform; check() asserts
the CONDITIONS of the case on them: what keeps a case from passing without reaching what it is there for."""
import functools

import numpy as np

from tests.synth_scene import TUM1, make_keyframes

F = np.float32
VOX = 4096
K31, K32 = 1 << 31, (1 << 32) - 1
COORD_LIMIT = 1 << 20                         # chunk ids the device holds: [-2^20, 2^20)


def small_cam(scale):
    c = dict(TUM1)
    for k in ("fx", "fy", "cx", "cy"):
        c[k] = c[k] / scale
    c["width"] //= scale
    c["height"] //= scale
    return c


def key_frame(seed, first=0):
    return make_keyframes(1, cam=small_cam(8), seed=seed, first=first)[0]


def rt(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)]).astype(F)


def rotation(w):
    """Rodrigues: axis * angle -> R"""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    k = w / max(th, 1e-12)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def small_motions(n, rng, rot=0.03, shift=0.08):
    return np.stack([rt(rotation(rng.normal(scale=rot, size=3)), rng.normal(scale=shift, size=3)) for _ in range(n)])


def quarter_turn(res):
    """Rz(90 deg), entries exactly 0 and +-1, and t = (res / 2, res / 2, 0): voxel centres land on voxel faces."""
    return rt([[0, -1, 0], [1, 0, 0], [0, 0, 1]], [F(res) * F(0.5), F(res) * F(0.5), 0])


def pack_rgbw(rgb, cw):
    rgb = rgb.astype(np.uint32)
    return (rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16) | (np.asarray(cw).astype(np.uint32) << 24)).astype(np.uint32)


def fill(rng, kfids=(0,), cw="random"):
    """One chunk: uniform weights 0.5 .. 3, normal sdf, random colours; kfid per voxel from `kfids`."""
    sdf = rng.normal(0.0, 0.05, VOX).astype(F)
    w = rng.uniform(0.5, 3.0, VOX).astype(F)
    kf = rng.choice(np.array(kfids, np.uint32), VOX)
    cws = rng.integers(0, 256, VOX) if cw == "random" else np.full(VOX, cw)
    return sdf, w, kf, pack_rgbw(rng.integers(0, 256, (VOX, 3)), cws)


def block(lo, shape):
    return [(lo[0] + x, lo[1] + y, lo[2] + z) for z in range(shape[2]) for y in range(shape[1]) for x in range(shape[0])]


# ------------------------------------------------------------------ the cases
def _mesh_and_integrate():
    """What follows a deform in the running system: the deformed chunks are meshed, the next cloud goes in."""
    return [("mesh",), ("integrate", key_frame(seed=139, first=1))]


def _collapse(res):
    rng = np.random.default_rng(101)
    chunks = [(cid, *fill(rng, (0, 1, 2), cw=0 if res == 0.05 else "random")) for cid in block((-1, -1, -1), (2, 2, 2))]
    r = F(res)
    quarter = rt(0.25 * np.eye(3), [r * F(8.3), r * F(7.9), r * F(9.1)])
    point = rt(np.zeros((3, 3)), [r * F(-20.5), r * F(3.5), r * F(40.5)])
    return dict(res=res, max_chunks=64,
                steps=[("upload", chunks), ("deform", "collapse", np.array([0, 1, 2], np.uint32), np.stack([quarter, quarter, point]))]
                + _mesh_and_integrate())


WEIGHT_CLASSES = {                      # name -> (value, is the voxel known: !((double)w <= 1e-15))
    "1e-15f": (F(1e-15), True),
    "below": (np.nextafter(F(1e-15), F(0)), False),
    "above": (np.nextafter(F(1e-15), F(1)), True),
    "zero": (F(0.0), False),
    "-zero": (F(-0.0), False),
    "-one": (F(-1.0), False),
    "subnormal": (np.frombuffer(np.uint32(1).tobytes(), F)[0], False),
    "1e-30": (F(1e-30), False),
    "one": (F(1.0), True),
    "1e29": (F(1e29), True),
}
CW_CLASSES = (0, 1, 253, 254, 255)
SDF_CLASSES = np.array([99999.0, 0.0, -0.0, 1e-5, -1e-5, 0.02, -0.03], F)
THRESHOLD_IDS = [(0, 0, 0), (-1, 0, 0), (0, -1, 1)]


def _thresholds():
    res = 0.05
    rng = np.random.default_rng(103)
    wv = np.array([v for v, _ in WEIGHT_CLASSES.values()], F)
    chunks = []
    for cid in THRESHOLD_IDS:
        w = wv[rng.integers(0, len(wv), VOX)]
        sdf = SDF_CLASSES[rng.integers(0, len(SDF_CLASSES), VOX)]
        cw = np.array(CW_CLASSES)[rng.integers(0, len(CW_CLASSES), VOX)]
        chunks.append((cid, sdf, w, rng.integers(0, 2, VOX).astype(np.uint32), pack_rgbw(rng.integers(0, 256, (VOX, 3)), cw)))
    q = quarter_turn(res)
    return dict(res=res, max_chunks=64,
                steps=[("upload", chunks), ("deform", "turn", np.array([0, 1], np.uint32), np.stack([q, q]))] + _mesh_and_integrate())


VOXEL_KFIDS = (0, 1, K31 - 1, K31, K32 - 1, K32, 12345)


def _kfid_map():
    res = 0.05
    rng = np.random.default_rng(107)
    ids = block((2, -3, 0), (2, 2, 1))

    def upload():
        out = []
        for cid in ids:
            sdf, w, kf, rgbw = fill(rng, VOXEL_KFIDS)
            w[rng.random(VOX) < 0.1] = 0                               # (so that "discarded" is not simply every voxel)
            out.append((cid, sdf, w, kf, rgbw))
        return ("upload", out)
    # (a) 5000 entries; of the voxels' kfids exactly 0 (first entry), 2^31 and 2^32 - 1 (last entry)
    pool = np.setdiff1d(np.unique(np.concatenate([rng.integers(2, K31 - 1, 3000), rng.integers(K31 + 1, K32 - 1, 3000)])),
                        np.array(VOXEL_KFIDS))
    big = np.sort(np.concatenate([rng.choice(pool, 4997, replace=False), [0, K31, K32]])).astype(np.uint32)
    assert len(big) == 5000 and np.all(np.diff(big.astype(np.int64)) > 0)
    assert sorted(set(big.tolist()) & set(VOXEL_KFIDS)) == [0, K31, K32] and big[0] == 0 and big[-1] == K32
    kf = key_frame(seed=109)
    one = small_motions(1, rng)
    return dict(res=res, max_chunks=256, steps=[
        ("deform", "never_filled", big, small_motions(5000, np.random.default_rng(1))),
        upload(), ("deform", "a", big, small_motions(5000, rng)),
        upload(), ("deform", "b", np.array([12345], np.uint32), one),
        upload(), ("deform", "c", np.zeros(0, np.uint32), np.zeros((0, 12), F)),
        ("integrate", kf), ("deform", "after_c", np.array([0], np.uint32), small_motions(1, rng)),
        upload(), ("deform", "d", np.array([2, 7, K31 + 5], np.uint32), small_motions(3, rng)),
    ])


def _sort_switch(which):
    res = 0.05
    rng = np.random.default_rng(113)
    if which == "above_2p20":
        chunks = [(cid, *fill(rng, (0, 1, 2))) for cid in block((-4, -3, -3), (8, 6, 6))]
        return dict(res=res, max_chunks=1024,
                    steps=[("upload", chunks), ("deform", "sort", np.arange(3, dtype=np.uint32), small_motions(3, rng, rot=0.05))])
    chunks = [(cid, *fill(rng)) for cid in block((-2, -2, -2), (4, 4, 4))]
    if which == "2p18_minus_1":
        chunks[37][2][1234] = 0
    return dict(res=res, max_chunks=512,
                steps=[("upload", chunks), ("deform", "sort", np.zeros(1, np.uint32), small_motions(1, rng, rot=0.05))])


def _far_block():
    res = 0.05
    rng = np.random.default_rng(127)
    chunks = [(cid, *fill(rng, (0, 1))) for cid in block((999, -701, 332), (2, 2, 2))]
    q = quarter_turn(res)
    return dict(res=res, max_chunks=64,
                steps=[("upload", chunks), ("deform", "turn", np.array([0, 1], np.uint32), np.stack([q, q]))] + _mesh_and_integrate())


def _far_edge():
    res = 0.05
    rng = np.random.default_rng(131)
    chunks = [(cid, *fill(rng)) for cid in [(COORD_LIMIT - 2, 0, -COORD_LIMIT), (COORD_LIMIT - 3, 1, -COORD_LIMIT + 1)]]
    r = F(res)
    shift = lambda k: rt(np.eye(3), [r * F(k), 0, 0])[None]
    kf = np.zeros(1, np.uint32)
    return dict(res=res, max_chunks=64,
                steps=[("upload", chunks), ("refuse", "plus32", kf, shift(32)), ("deform", "plus16", kf, shift(16))])


CAPACITY_N = 14                                # a 6 x 2 x 1 block moved by half a chunk along x: 7 x 2 x 1


def _capacity(short):
    res = 0.05
    rng = np.random.default_rng(137)
    chunks = [(cid, *fill(rng)) for cid in block((-3, 0, 1), (6, 2, 1))]
    r = F(res)
    kf = np.zeros(1, np.uint32)
    half, whole = rt(np.eye(3), [r * F(8), 0, 0])[None], rt(np.eye(3), [r * F(16), 0, 0])[None]
    if short:
        return dict(res=res, max_chunks=CAPACITY_N - 1,
                    steps=[("upload", chunks), ("refuse", "half", kf, half), ("deform", "whole", kf, whole),
                           ("refuse", "half_again", kf, half), ("deform", "whole_again", kf, whole)])
    return dict(res=res, max_chunks=CAPACITY_N, steps=[("upload", chunks), ("deform", "half", kf, half)])


BUILDERS = {
    "collapse_5cm": lambda: _collapse(0.05),
    "collapse_10cm": lambda: _collapse(0.1),
    "thresholds": _thresholds,
    "kfid_map": _kfid_map,
    "sort_2p18": lambda: _sort_switch("2p18"),
    "sort_2p18_minus_1": lambda: _sort_switch("2p18_minus_1"),
    "sort_above_2p20": lambda: _sort_switch("above_2p20"),
    "far_block": _far_block,
    "far_edge": _far_edge,
    "capacity_met": lambda: _capacity(False),
    "capacity_short": lambda: _capacity(True),
}
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case, built once per process.  Callers do not write into its arrays."""
    return BUILDERS[name]()


# ------------------------------------------------------------------ the reference's walk, restated on a map's voxels
def walk(m, res, kfids, Rt):
    """The records ChunkManager::Deform would make of map `m` (chunk_order(), get_chunk): one per moving voxel, in the
    reference's sequence (chunks in container order, voxels by id), with the float32 arithmetic of :972-977 and
    Chunk.cpp:101-105.  -> dict(moved, discarded, undefined, new_ids (first-claim order), key [moved] (dense index of
    the new voxel), at [moved] (entry of the deformation map), cw [moved] (colour weight of the old voxel))."""
    kfids = np.ascontiguousarray(kfids, np.uint32)
    Rt = np.ascontiguousarray(Rt, F).reshape(len(kfids), 12)
    r = F(res)
    half, inv_res, rounding = r * F(0.5), F(1.0) / r, F(1.0) / (F(16.0) * r)
    lx, ly, lz = (np.arange(VOX) & 15).astype(F), ((np.arange(VOX) >> 4) & 15).astype(F), (np.arange(VOX) >> 8).astype(F)
    ids, vox, ats, cws = [], [], [], []
    discarded = 0
    for cid in m.chunk_order():
        _, w, kf, rgbw = m.get_chunk(*cid)
        known = ~(w.astype(np.float64) <= 1e-15)
        at = np.searchsorted(kfids, kf)
        hit = np.zeros(VOX, bool)
        if len(kfids):
            hit = kfids[np.minimum(at, len(kfids) - 1)] == kf
        discarded += int((known & ~hit).sum())
        mv = known & hit
        if not mv.any():
            continue
        a = at[mv]
        p = [(l[mv] * r + half) + F(16 * int(c)) * r for l, c in zip((lx, ly, lz), cid)]
        R = Rt[a]
        q = [R[:, 9 + i] + (R[:, 3 * i] * p[0] + (R[:, 3 * i + 1] * p[1] + R[:, 3 * i + 2] * p[2])) for i in range(3)]
        assert all(x.dtype == F for x in q)
        nid = np.stack([np.floor(x * rounding).astype(np.int64) for x in q], -1)
        g = np.stack([np.floor(x * inv_res).astype(np.int64) for x in q], -1)
        loc = g - 16 * nid
        ids.append(nid)
        vox.append((loc[:, 2] * 16 + loc[:, 1]) * 16 + loc[:, 0])
        ats.append(a)
        cws.append((rgbw[mv] >> 24).astype(np.int64))
    if not ids:
        z = np.zeros(0, np.int64)
        return dict(moved=0, discarded=discarded, undefined=0, new_ids=[], key=z, at=z, cw=z)
    ids, vox, ats, cws = np.concatenate(ids), np.concatenate(vox), np.concatenate(ats), np.concatenate(cws)
    uniq, first, inv = np.unique(ids, axis=0, return_index=True, return_inverse=True)
    new_ids = [tuple(int(v) for v in uniq[i]) for i in np.argsort(first)]
    ok = (vox >= 0) & (vox < VOX)
    key = np.where(ok, inv.reshape(-1) * VOX + vox, -1)
    return dict(moved=len(vox), discarded=discarded, undefined=int((~ok).sum()), new_ids=new_ids, key=key, at=ats, cw=cws)


def runs(w):
    """-> (claimants per new voxel, record index of each new voxel's first claimant)"""
    key = w["key"][w["key"] >= 0]
    if not len(key):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    _, first, count = np.unique(key, return_index=True, return_counts=True)
    return count, np.flatnonzero(w["key"] >= 0)[first]


def apply_step(m, step):
    """One step on an oracle map with track_order(); a refused deform leaves it alone."""
    if step[0] == "upload":
        for cid, *planes in step[1]:
            m.set_chunk(*cid, *planes)
    elif step[0] == "integrate":
        kf = step[1]
        m.integrate(kf["xyz"], kf["rgb"], kf["kfid"], kf["Twc"])
        m.end_call()
    elif step[0] == "deform":
        return m.deform(step[2], step[3])
    return None


def map_voxels(m):
    ids = [tuple(int(v) for v in c) for c in m.chunk_ids()]
    return {cid: m.get_chunk(*cid) for cid in ids}


def measure(oracle, c):
    """The case on the oracle alone -> {tag: counters of that deform}.  A refused deform is measured on a second map
    that replays the steps before it."""
    m = oracle.chisel(c["res"]).track_order()
    out = {}
    for i, step in enumerate(c["steps"]):
        if step[0] == "refuse":
            scratch = oracle.chisel(c["res"]).track_order()
            for s in c["steps"][:i]:
                apply_step(scratch, s)
            n_new, _, _ = scratch.deform(step[2], step[3])
            out[step[1]] = dict(refused=True, new_chunks=n_new, ids=[tuple(int(v) for v in x) for x in scratch.chunk_ids()])
            scratch.close()
            continue
        if step[0] != "deform":
            apply_step(m, step)
            continue
        before = map_voxels(m)
        w = walk(m, c["res"], step[2], step[3])
        n_new, discarded, undefined = apply_step(m, step)
        after = map_voxels(m)
        # the restated walk and the oracle agree on every counter: the class counters below speak about the oracle's run
        assert (w["discarded"], w["undefined"]) == (discarded, undefined) and set(w["new_ids"]) == set(after) and n_new == len(after)
        assert set(map(tuple, m.chunk_order().tolist())) == set(after)
        count, first = runs(w)
        known_before = sum(int((~(v[1].astype(np.float64) <= 1e-15)).sum()) for v in before.values())
        cw_after = np.concatenate([v[3] >> 24 for v in after.values()]) if after else np.zeros(0, np.uint32)
        finite = all(np.isfinite(v[0]).all() and np.isfinite(v[1]).all() for v in after.values())
        out[step[1]] = dict(refused=False, new_chunks=n_new, discarded=discarded, undefined=undefined, moved=w["moved"],
                            known_before=known_before, chunks_before=len(before), ids=sorted(after), finite=finite,
                            longest_run=int(count.max()) if len(count) else 0, new_voxels=len(count),
                            shared=float((count >= 2).mean()) if len(count) else 0.0,
                            at_cw254=int((cw_after == 254).sum()),
                            # runs whose later claimants outnumber the colour updates left below 254 (all weights known)
                            freeze_discards=int((count - 1 > np.maximum(254 - w["cw"][first], 0)).sum()) if len(count) else 0,
                            cw_first=sorted(set(w["cw"][first].tolist())) if len(count) else [],
                            cw_later=sorted(set(np.delete(w["cw"], first).tolist())) if len(count) else [],
                            at_hit=np.unique(w["at"]).tolist())
    m.close()
    return out


def weight_class_counts(c):
    w = np.concatenate([ch[2] for ch in c["steps"][0][1]]).view(np.uint32)
    return {name: int((w == np.array([v], F).view(np.uint32)[0]).sum()) for name, (v, _) in WEIGHT_CLASSES.items()}


def check(name, c, got):
    """The conditions of case `name` on measure()'s counters."""
    for tag, g in got.items():
        if not g["refused"]:
            assert g["undefined"] == 0, (name, tag)
            assert g["new_chunks"] <= c["max_chunks"], (name, tag)
    if name.startswith("collapse"):
        g = got["collapse"]
        assert g["longest_run"] > 10000 and g["at_cw254"] >= 1 and g["freeze_discards"] >= 1 and g["new_chunks"] <= 8, g
    elif name == "thresholds":
        g = got["turn"]
        counts = weight_class_counts(c)
        assert all(n >= 20 for n in counts.values()), counts
        known = sum(n for k, n in counts.items() if WEIGHT_CLASSES[k][1])
        assert g["known_before"] == known == g["moved"] and g["discarded"] == 0        # the threshold, class by class
        assert set(CW_CLASSES) <= set(g["cw_first"]) and set(CW_CLASSES) <= set(g["cw_later"]), g
        assert g["finite"]
        for ch in c["steps"][0][1]:
            assert np.isfinite(ch[2]).all() and np.isfinite(ch[1]).all()
    elif name == "kfid_map":
        assert got["never_filled"]["chunks_before"] == 0
        assert (got["never_filled"]["moved"], got["never_filled"]["new_chunks"], got["never_filled"]["discarded"]) == (0, 0, 0)
        a = got["a"]
        assert a["discarded"] > 0 and a["moved"] > 0 and {0, 4999} <= set(a["at_hit"]), a
        assert len(a["at_hit"]) == 3
        assert got["b"]["moved"] > 0 and got["b"]["at_hit"] == [0]
        for tag in ("c", "d"):
            g = got[tag]
            assert g["moved"] == 0 and g["new_chunks"] == 0 and g["discarded"] == g["known_before"] > 0 and g["ids"] == [], (tag, g)
        assert got["after_c"]["moved"] > 0 and got["after_c"]["new_chunks"] > 0
    elif name.startswith("sort_"):
        g = got["sort"]
        want = {"sort_2p18": 1 << 18, "sort_2p18_minus_1": (1 << 18) - 1, "sort_above_2p20": 288 * VOX}[name]
        assert g["moved"] == want and g["discarded"] == 0, g
        if name == "sort_above_2p20":
            assert want == 1179648 > 1 << 20 and g["shared"] >= 0.30, g
    elif name == "far_block":
        g = got["turn"]
        assert g["moved"] == 8 * VOX and g["new_chunks"] >= 8 and min(max(abs(v) for v in cid) for cid in g["ids"]) >= 600, g
    elif name == "far_edge":
        g = got["plus16"]
        assert g["new_chunks"] >= 1 and any(cid[0] == COORD_LIMIT - 1 for cid in g["ids"]), g
        assert all(-COORD_LIMIT <= v < COORD_LIMIT for cid in g["ids"] for v in cid), g
        assert any(v >= COORD_LIMIT for cid in got["plus32"]["ids"] for v in cid), got["plus32"]
        assert got["plus32"]["new_chunks"] <= c["max_chunks"]            # the range alone is what the device refuses
    elif name == "capacity_met":
        assert CAPACITY_N >= 12 and got["half"]["new_chunks"] == CAPACITY_N == c["max_chunks"]
    elif name == "capacity_short":
        for refused, done in (("half", "whole"), ("half_again", "whole_again")):     # (the second pair: after a deform that went through)
            assert got[refused]["new_chunks"] == CAPACITY_N == c["max_chunks"] + 1
            assert 0 < got[done]["new_chunks"] <= c["max_chunks"] and got[done]["moved"] == 12 * VOX
    else:
        raise AssertionError(name)
