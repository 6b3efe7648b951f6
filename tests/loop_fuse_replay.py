"""A toy map for the replay rule of INTEGRATION.md 2l ("LoopClosing::SearchAndFuse through LoopFuseSearch"): the map of
tests/orb_fuse_replay.py — per point its observations, descriptor and bad flag, per key frame its slots, with MapPoint::AddObservation,
Replace (reference src/MapPoint.cc:306-360) and ComputeDistinctiveDescriptors as the search stage's caller sees them — under the Sim3
overload's tail (src/ORBmatcher.cc:1535-1548: vpReplacePoint[i] is FILLED during the loop) and SearchAndFuse's Replace loop after it
(src/LoopClosing.cc:3197-3206: pRep->Replace(vpMapPoints[i]), the LOOP point survives).

sequential(): the reference's two loops — key frame after key frame: the snapshot spAlreadyFound, every loop point searched with LIVE
data at the moment the reference would reach it, then the Replace loop.
replayed(): ONE batched search taken before any mutation, then the same loops with the rule: per key frame take the snapshot live,
re-test isBad() / the snapshot live, take the batch's candidate unless the point is dirty, re-query a dirty point for that key frame
with its live descriptor, apply :1535-1548, and after the key frame run the Replace loop and mark every survivor dirty."""
import copy

import numpy as np

from tests import loop_fuse_scenario as S
from tests import orb_fuse_replay as P
from tests import orb_fuse_scenario as PS


class LoopMap(P.ToyMap):
    def loop_fuse_tail(self, k, pid, best_idx, replace_with):
        """src/ORBmatcher.cc:1535-1548."""
        other = int(self.slots[k][best_idx])
        if other >= 0:
            if not self.bad[other]:
                replace_with[pid] = other
        else:
            self.add_observation(pid, k, best_idx)
            self.slots[k][best_idx] = pid

    def replace_loop(self, loop_ids, replace_with):
        """src/LoopClosing.cc:3197-3206 -> the survivors, in order."""
        out = []
        for i in loop_ids:
            if i in replace_with:
                self.replace(replace_with[i], i)
                out.append(i)
        return out


def replay_inputs():
    """tests/orb_fuse_replay.replay_inputs() under Sim3 poses, its current points as the loop points.  Loop point 2 is made a twin of
    loop point 1 (the same world point, a descriptor two bits off): in key frame 0, where their key point carries no map point, point
    1 takes the slot (AddMapPoint) and point 2, finding point 1 there, asks for its replacement."""
    inp = P.replay_inputs()
    K, M = inp["K"], inp["M"]
    rng = np.random.default_rng(S.SEED + 5)
    pts, tmap = inp["points"], inp["map"]
    for k in ("pos", "normal", "min_dist", "max_dist"):
        pts[k][2] = pts[k][1]
    pts["desc"][2] = PS._flip(rng, pts["desc"][1], 2)
    tmap.desc[K][2] = pts["desc"][2]
    tmap.compute_distinctive_descriptors(2)
    lmap = LoopMap.__new__(LoopMap)
    lmap.__dict__.update(copy.deepcopy(tmap.__dict__))
    return dict(kfs=S._as("points", inp["kfs"], S.SCALES), points=pts, map=lmap, th=S.TH, M=M, K=K)


def _snapshot(tmap, k):
    return {int(p) for p in tmap.slots[k] if p >= 0}


def _skip(tmap, K, M):
    return np.array([[tmap.bad[i] or i in _snapshot(tmap, k) for i in range(M)] for k in range(K)], np.uint8)


def sequential(inp, search):
    """search(kfs, points, skip) -> best_idx [len(kfs), m].  Every pair with live data, in the reference's order."""
    tmap = copy.deepcopy(inp["map"])
    ids = list(range(inp["M"]))
    for k in range(inp["K"]):
        already, replace_with = _snapshot(tmap, k), {}
        for i in ids:
            if tmap.bad[i] or i in already:
                continue
            best = int(search([inp["kfs"][k]], P._live_points(inp["points"], tmap, [i]), None)[0, 0])
            if best >= 0:
                tmap.loop_fuse_tail(k, i, best, replace_with)
        tmap.replace_loop(ids, replace_with)
    return tmap


def replayed(inp, search, batch_search=None, log=None, requery=True):
    """One batched search (batch_search, default = search) before any mutation, then the replay.  requery=False leaves the rule's
    re-query of dirty points out (to show that it is needed)."""
    tmap = copy.deepcopy(inp["map"])
    K, M = inp["K"], inp["M"]
    ids = list(range(M))
    batch = (batch_search or search)(inp["kfs"], P._live_points(inp["points"], tmap, ids), _skip(tmap, K, M))
    dirty = set()
    for k in range(K):
        already, replace_with = _snapshot(tmap, k), {}
        for i in ids:
            if tmap.bad[i] or i in already:          # live: they only ever remove pairs
                continue
            best = int(batch[k, i])
            if i in dirty:
                live = int(search([inp["kfs"][k]], P._live_points(inp["points"], tmap, [i]), None)[0, 0])
                if log is not None:
                    log.append((k, i, best, live))
                if requery:
                    best = live
            if best >= 0:
                tmap.loop_fuse_tail(k, i, best, replace_with)
        dirty.update(tmap.replace_loop(ids, replace_with))
    return tmap


class Searcher:
    """search(kfs, points, skip) over resident handles: one handle per key frame dictionary, made on first sight and kept."""

    def __init__(self, host):
        self.host, self.made = host, {}

    def __call__(self, kfs, items, skip):
        from plvs_amd.keyframe import ResidentKeyFrame, loop_fuse_search_kf
        views, packed = PS.views({"kfs": kfs, "points": items})
        hs = []
        for kf, v in zip(kfs, views):
            if id(kf) not in self.made:
                self.made[id(kf)] = ResidentKeyFrame(points=v, host_only=self.host)
            hs.append(self.made[id(kf)])
        return loop_fuse_search_kf(hs, S.poses(kfs), packed, S.TH, skip, host=self.host)["best_idx"]

    def close(self):
        for h in self.made.values():
            h.close()
