"""A toy map for the replay rule of INTEGRATION.md 2j ("SearchInNeighbors through LineMatcher::FuseSearch"): per line its
observations, descriptor and bad flag, per key frame its slots, with MapLine::AddObservation (reference src/MapLine.cc:231-263: an
observation with both right abscissae counts twice), Replace (:371-473 with USE_ENDPOINTS_AVERAGING 0: no end point, normal or
mfMaxDistance moves) and ComputeDistinctiveDescriptors (:505-585, the least median of the pairwise distances, first minimum) as the
search stage's caller sees them, and LineMatcher::Fuse's tail (src/LineMatcher.cc:2279-2306).  The map's bookkeeping is the toy map
of tests/orb_fuse_replay.py: the two classes keep the same books.

sequential(): the reference's forward loop of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:1434-1440) — key frame after key
frame, line after line, every pair searched with LIVE data at the moment the reference would reach it.
replayed(): ONE batched search taken before any mutation, then the same loops with the rule: re-test isBad / IsInKeyFrame live, take
the batch's candidate unless the line is dirty, re-query a dirty line for that key frame with its live descriptor, apply
:2279-2306, mark the survivor of every Replace dirty."""
import copy

import numpy as np

from tests import line_fuse_scenario as S
from tests.orb_fuse_replay import ToyMap

f32 = np.float32


class ToyLineMap(ToyMap):
    def __init__(self, kfs, cur_desc, cur_stereo):
        self.desc = [np.asarray(kf["desc"], np.uint8) for kf in kfs] + [np.asarray(cur_desc, np.uint8)]
        both = lambda kf: (np.zeros(len(kf["kl"]), bool) if kf["u_right_start"] is None
                           else (np.asarray(kf["u_right_start"], f32) >= 0) & (np.asarray(kf["u_right_end"], f32) >= 0))
        self.stereo = [both(kf) for kf in kfs] + [np.asarray(cur_stereo, bool)]
        self.slots = [np.full(len(d), -1, np.int64) for d in self.desc]
        self.obs, self.n_obs, self.bad, self.point_desc = {}, {}, {}, {}
        self.replacements = []                                   # (the line that went bad, the survivor)


def _project(kf, w):
    Rm = np.asarray(kf["Rcw"], np.float64).reshape(3, 3).T
    pc = w @ Rm.T + kf["tcw"].astype(np.float64)
    K = kf["K4"].astype(np.float64)
    return K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3], pc[:, 2]


def replay_inputs(K=3, N=90, M=60, seed=11):
    """K target key frames that all see the same N world lines (each with its own few-bit variant of the line's descriptor, in its
    own key line order) and a current key frame whose M map lines are the first M of them.  Every third line's slot in key frame 0
    is held by an old map line, seen without right abscissae: one with a second observation in key frame 1 (2 observations against
    the 2 of a current line seen in stereo: `>` fails, the current line survives the Replace, takes both observations and a new
    descriptor — it is dirty for key frame 2), the next with observations in all three (3 against 1: the old line survives).  The
    descriptors of the current lines whose slot is held lie 55 bits from the world line's, the key frames' 8: around TH_LOW (60)
    from each other, so that some are fused in key frame 0 and, with the stale descriptor, not found in key frame 2."""
    rng = np.random.default_rng(S.SEED + seed)
    poses = S._poses(K)
    empty = lambda Rm, t: S.make_kf(Rm, t, S.keylines(np.zeros((0, 4)), 0), np.zeros((0, 32), np.uint8), None, None)
    ref = empty(*poses[0])
    # (apart, so that the gates admit one world line)
    cx, cy = 70 + (np.arange(N) % 9) * 60.0 + rng.uniform(-5, 5, N), 50 + (np.arange(N) // 9) * 42.0 + rng.uniform(-5, 5, N)
    segs = np.stack([S.seg_at(float(a), float(x), float(y), 22.0) for a, x, y in zip(rng.uniform(-80, 80, N), cx, cy)])
    zs, ze = rng.uniform(1.5, 3.0, N), rng.uniform(1.5, 3.0, N)
    ws = np.stack([S.world(ref, s[0], s[1], z) for s, z in zip(segs, zs)])
    we = np.stack([S.world(ref, s[2], s[3], z) for s, z in zip(segs, ze)])
    base = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    kfs, slot_of = [], []
    for k, (Rm, t) in enumerate(poses):
        kf = empty(Rm, t)
        xs, ys, zzs = _project(kf, ws)
        xe, ye, zze = _project(kf, we)
        perm = rng.permutation(N)                           # key line slot s shows world line perm[s]
        inv = np.argsort(perm)
        none = (rng.random(N) < 0.5) | ((np.arange(N) % 3 == 0) & (np.arange(N) < M))
        urs, ure = np.where(none, -1.0, xs - float(S.MBF) / zzs), np.where(none, -1.0, xe - float(S.MBF) / zze)
        desc = np.array([S._flip(rng, base[j], 8) for j in range(N)], np.uint8)
        kl = S.keylines(np.stack([xs, ys, xe, ye], 1)[perm], 1)
        kfs.append(S.make_kf(Rm, t, kl, desc[perm], urs[perm], ure[perm]))
        slot_of.append(inv)
    bits = [55, 24, 30]       # (every third line, the ones whose slot in key frame 0 is held: ~60 bits from a key frame's variant)
    lines = []
    for i in range(M):
        Mw = 0.5 * (ws[i] + we[i])
        PO = Mw - kfs[0]["Ow"].astype(np.float64)
        Rm = np.asarray(kfs[0]["Rcw"], np.float64).reshape(3, 3).T
        dist = np.linalg.norm(Rm @ Mw + kfs[0]["tcw"].astype(np.float64))
        lines.append((ws[i].astype(f32), we[i].astype(f32), (PO / np.linalg.norm(PO)).astype(f32), f32(dist * 1.2 ** 0.5),
                      S._flip(rng, base[i], bits[i % 3])))
    lines = S._pack(lines)
    tmap = ToyLineMap(kfs, lines["desc"], np.arange(M) % 6 == 0)
    for i in range(M):
        tmap.new_point(i, [(K, i)])
    old = M
    for i in range(0, M, 3):
        obs = [(0, int(slot_of[0][i])), (1, int(slot_of[1][i]))] + ([(2, int(slot_of[2][i]))] if i % 2 else [])
        tmap.new_point(old, obs)
        old += 1
    return dict(kfs=kfs, lines=lines, map=tmap, th=S.TH, M=M, K=K)


def _skip(tmap, K, M):
    return np.array([[tmap.bad[i] or k in tmap.obs[i] for i in range(M)] for k in range(K)], np.uint8)


def _live_lines(lines, tmap, ids):
    p = {k: np.ascontiguousarray(lines[k][ids]) for k in ("start", "end", "normal", "max_dist")}
    p["desc"] = np.array([tmap.point_desc[i] for i in ids], np.uint8).reshape(-1, 32)
    return p


def sequential(inp, search):
    """search(kfs, lines, skip) -> best_idx [len(kfs), m].  Every pair with live data, in the reference's order."""
    tmap = copy.deepcopy(inp["map"])
    for k in range(inp["K"]):
        for i in range(inp["M"]):
            if tmap.bad[i] or k in tmap.obs[i]:
                continue
            best = int(search([inp["kfs"][k]], _live_lines(inp["lines"], tmap, [i]), None)[0, 0])
            if best >= 0:
                tmap.fuse_tail(k, i, best)
    return tmap


def replayed(inp, search, batch_search=None, log=None, requery=True):
    """One batched search (batch_search, default = search) before any mutation, then the replay.  requery=False leaves the rule's
    re-query of dirty lines out (to show that it is needed)."""
    tmap = copy.deepcopy(inp["map"])
    K, M = inp["K"], inp["M"]
    batch = (batch_search or search)(inp["kfs"], _live_lines(inp["lines"], tmap, list(range(M))), _skip(tmap, K, M))
    dirty = set()
    for k in range(K):
        for i in range(M):
            if tmap.bad[i] or k in tmap.obs[i]:        # live: they only ever remove pairs
                continue
            best = int(batch[k, i])
            if i in dirty:
                live = int(search([inp["kfs"][k]], _live_lines(inp["lines"], tmap, [i]), None)[0, 0])
                if log is not None:
                    log.append((k, i, best, live))
                if requery:
                    best = live
            if best >= 0:
                survivor = tmap.fuse_tail(k, i, best)
                if survivor is not None:
                    dirty.add(survivor)
    return tmap
