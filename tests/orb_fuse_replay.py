"""A toy map for the replay rule of INTEGRATION.md ("SearchInNeighbors through ORBmatcher::FuseSearch"): per point its observations,
descriptor and bad flag, per key frame its slots, with MapPoint::AddObservation (reference src/MapPoint.cc:177-202), Replace
(:306-360) and ComputeDistinctiveDescriptors (:389-463, the least median of the pairwise distances, first minimum) as the search
stage's caller sees them, and ORBmatcher::Fuse's tail (src/ORBmatcher.cc:1408-1427).

sequential(): the reference's forward loop of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:1375-1381) — key frame after key
frame, point after point, every pair searched with LIVE data at the moment the reference would reach it.
replayed(): ONE batched search taken before any mutation, then the same loops with the rule: re-test isBad / IsInKeyFrame live, take
the batch's candidate unless the point is dirty, re-query a dirty point for that key frame with its live descriptor, apply
:1408-1427, mark the survivor of every Replace dirty."""
import copy

import numpy as np

from tests import orb_fuse_scenario as S

f32 = np.float32
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


class ToyMap:
    def __init__(self, kfs, cur_desc, cur_stereo):
        """kfs: the target key frames (scenario dicts); the current key frame is index len(kfs) and holds `cur_desc` [M, 32];
        cur_stereo [M]: its key point has a right coordinate (an observation there counts twice)."""
        self.desc = [np.asarray(kf["desc"], np.uint8) for kf in kfs] + [np.asarray(cur_desc, np.uint8)]
        self.stereo = [np.asarray(kf["u_right"], f32) >= 0 for kf in kfs] + [np.asarray(cur_stereo, bool)]
        self.slots = [np.full(len(d), -1, np.int64) for d in self.desc]
        self.obs, self.n_obs, self.bad, self.point_desc = {}, {}, {}, {}
        self.replacements = []                                   # (the point that went bad, the survivor)

    def new_point(self, pid, observations):
        self.obs[pid], self.n_obs[pid], self.bad[pid], self.point_desc[pid] = {}, 0, False, None
        for k, idx in observations:
            self.add_observation(pid, k, idx)
            self.slots[k][idx] = pid
        self.compute_distinctive_descriptors(pid)

    def add_observation(self, pid, k, idx):                      # :177-202 (no second camera)
        self.obs[pid][k] = idx
        self.n_obs[pid] += 2 if self.stereo[k][idx] else 1

    def compute_distinctive_descriptors(self, pid):              # :389-463; std::map order = key frame order
        if self.bad[pid] or not self.obs[pid]:
            return
        d = np.array([self.desc[k][idx] for k, idx in sorted(self.obs[pid].items())], np.uint8)
        n = len(d)
        dist = _POP[d[:, None, :] ^ d[None, :, :]].sum(-1)
        med = np.sort(dist, 1)[:, int(0.5 * (n - 1))]
        self.point_desc[pid] = d[int(np.argmin(med))].copy()     # median < BestMedian: the first minimum

    def replace(self, pid, by):                                  # pid->Replace(by), :306-360
        if pid == by:
            return
        obs, self.obs[pid], self.bad[pid] = self.obs[pid], {}, True
        self.replacements.append((pid, by))
        for k, idx in sorted(obs.items()):
            if k not in self.obs[by]:
                self.slots[k][idx] = by
                self.add_observation(by, k, idx)
            else:
                self.slots[k][idx] = -1
        self.compute_distinctive_descriptors(by)

    def fuse_tail(self, k, pid, best_idx):
        """src/ORBmatcher.cc:1408-1427 -> the survivor of a Replace, or None."""
        other = int(self.slots[k][best_idx])
        if other >= 0:
            if self.bad[other]:
                return None
            if self.n_obs[other] > self.n_obs[pid]:
                self.replace(pid, other)
                return other
            self.replace(other, pid)
            return pid
        self.add_observation(pid, k, best_idx)
        self.slots[k][best_idx] = pid
        return None

    def state(self):
        return dict(slots=[s.tolist() for s in self.slots], obs={p: sorted(o.items()) for p, o in self.obs.items()}, n_obs=dict(self.n_obs),
                    bad=dict(self.bad), desc={p: None if d is None else d.tobytes() for p, d in self.point_desc.items()})


def replay_inputs(K=3, N=90, M=60, seed=11):
    """K target key frames that all see the same N world points (each with its own few-bit variant of the point's descriptor, in its
    own key point order) and a current key frame whose M map points are the first M of them.  Every third point's slot in key frame
    0 is held by an old map point, seen without a right coordinate: one with a second observation in key frame 1 (2 observations
    against the 2 of a current point seen in stereo: `>` fails, the current point survives the Replace, takes both observations and a
    new descriptor — it is dirty for key frame 2), the next with observations in all three (3 against 1: the old point survives).
    The current points' descriptors lie 20 to 45 bits from the world point's, the key frames' 8: around TH_LOW from each other."""
    rng = np.random.default_rng(S.SEED + seed)
    poses = S._poses(K)
    ref = S.make_kf(poses[0][0], poses[0][1], [], [], [], [], np.zeros((0, 32), np.uint8))
    # (apart, so that a window holds one world point)
    u, v = 60 + (np.arange(N) % 10) * 55.0 + rng.uniform(-5, 5, N), 60 + (np.arange(N) // 10) * 42.0 + rng.uniform(-5, 5, N)
    depth = rng.uniform(1.5, 3.0, N)
    world = S.world(ref, u, v, depth)
    base = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    octave = rng.integers(1, S.N_LEVELS - 1, N)
    kfs, slot_of = [], []
    for k, (q, t) in enumerate(poses):
        kf = S.make_kf(q, t, [], [], [], [], np.zeros((0, 32), np.uint8))
        from tests.track_motion_restatement import se3_act
        pc = se3_act(q, t, world).astype(np.float64)
        x, y = S.K4[0] * pc[:, 0] / pc[:, 2] + S.K4[2], S.K4[1] * pc[:, 1] / pc[:, 2] + S.K4[3]
        perm = rng.permutation(N)                           # key point perm[s] ... slot s shows world point perm[s]
        inv = np.argsort(perm)
        ur = np.where((rng.random(N) < 0.5) | ((np.arange(N) % 3 == 0) & (np.arange(N) < M)), -1.0, x - float(S.MBF) / pc[:, 2])
        desc = np.array([S._flip(rng, base[j], 8) for j in range(N)], np.uint8)
        kfs.append(S.make_kf(q, t, x[perm], y[perm], octave[perm], ur[perm], desc[perm]))
        slot_of.append(inv)
    pts = []
    bits = [20, 41, 43, 45]
    for i in range(M):
        PO = world[i].astype(np.float64) - kfs[0]["Ow"].astype(np.float64)
        dist = np.linalg.norm(PO)
        max_dist = f32(dist * 1.2 ** (int(octave[i]) - 0.5))
        pts.append((world[i], (PO / dist).astype(f32), f32(max_dist / 1.2 ** (S.N_LEVELS - 1)), max_dist, S._flip(rng, base[i], bits[i % 4])))
    points = S._pack(pts)
    tmap = ToyMap(kfs, points["desc"], np.arange(M) % 6 == 0)
    for i in range(M):
        tmap.new_point(i, [(K, i)])
    old = M
    for i in range(0, M, 3):
        obs = [(0, int(slot_of[0][i])), (1, int(slot_of[1][i]))] + ([(2, int(slot_of[2][i]))] if i % 2 else [])
        tmap.new_point(old, obs)
        old += 1
    return dict(kfs=kfs, points=points, map=tmap, th=S.TH, M=M, K=K)


def _skip(tmap, K, M):
    return np.array([[tmap.bad[i] or k in tmap.obs[i] for i in range(M)] for k in range(K)], np.uint8)


def _live_points(points, tmap, ids):
    p = {k: np.ascontiguousarray(points[k][ids]) for k in ("pos", "normal", "min_dist", "max_dist")}
    p["desc"] = np.array([tmap.point_desc[i] for i in ids], np.uint8).reshape(-1, 32)
    return p


def sequential(inp, search):
    """search(kfs, points, skip) -> best_idx [len(kfs), m].  Every pair with live data, in the reference's order."""
    tmap = copy.deepcopy(inp["map"])
    for k in range(inp["K"]):
        for i in range(inp["M"]):
            if tmap.bad[i] or k in tmap.obs[i]:
                continue
            best = int(search([inp["kfs"][k]], _live_points(inp["points"], tmap, [i]), None)[0, 0])
            if best >= 0:
                tmap.fuse_tail(k, i, best)
    return tmap


def replayed(inp, search, batch_search=None, log=None, requery=True):
    """One batched search (batch_search, default = search) before any mutation, then the replay.  requery=False leaves the rule's
    re-query of dirty points out (to show that it is needed)."""
    tmap = copy.deepcopy(inp["map"])
    K, M = inp["K"], inp["M"]
    batch = (batch_search or search)(inp["kfs"], _live_points(inp["points"], tmap, list(range(M))), _skip(tmap, K, M))
    dirty = set()
    for k in range(K):
        for i in range(M):
            if tmap.bad[i] or k in tmap.obs[i]:        # live: they only ever remove pairs
                continue
            best = int(batch[k, i])
            if i in dirty:
                live = int(search([inp["kfs"][k]], _live_points(inp["points"], tmap, [i]), None)[0, 0])
                if log is not None:
                    log.append((k, i, best, live))
                if requery:
                    best = live
            if best >= 0:
                survivor = tmap.fuse_tail(k, i, best)
                if survivor is not None:
                    dirty.add(survivor)
    return tmap
