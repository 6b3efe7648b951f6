"""Helpers of the resident key-frame tests (tests/test_keyframe_resident.py, tests/test_keyframe_resident_gpu.py): handles from the
scenario dictionaries of tests/orb_fuse_scenario.py and tests/line_fuse_scenario.py, searches over them shaped like the tests' _search
of the non-resident entries, and the overwriting of a scenario's source arrays."""
import numpy as np

from tests import line_fuse_scenario as LS
from tests import orb_fuse_scenario as PS

OUTPUTS = ("best_idx", "best_dist", "reached")
POINT_ARRAYS = ("x", "y", "octave", "u_right", "desc", "scale_factors", "inv_level_sigma2", "K4", "bounds4")
LINE_ARRAYS = ("kl", "desc", "u_right_start", "u_right_end", "scale_factors", "inv_level_sigma2", "K4", "bounds4")


def same(out, want, keys=OUTPUTS, what=""):
    for k in keys:
        a, b = np.asarray(out[k]), np.asarray(want[k])
        assert a.shape == b.shape and (a == b).all(), f"{what}{k} differs at {np.argwhere(a != b)[:8].tolist()}"


def own_copy(inp):
    """The scenario with arrays of its own (the scenarios share module-level tables such as SCALE_FACTORS)."""
    out = dict(inp)
    out["kfs"] = [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in kf.items()} for kf in inp["kfs"]]
    return out


def smash(inp, names):
    """0xFF into every byte of every source array of every key frame (the arrays the views hold are these very arrays or, where a
    conversion was needed, copies made by as_c() that die with the view)."""
    for kf in inp["kfs"]:
        for k in names:
            if kf[k] is not None:
                kf[k].view(np.uint8).reshape(-1)[:] = 0xFF


class Handles:
    """Handles of a point or a line scenario (or of both: the same key-frame list for both kinds), their poses, closed on exit."""

    def __init__(self, points_inp=None, lines_inp=None, host_only=False, smash_sources=False):
        from plvs_amd.keyframe import KeyFramePose, ResidentKeyFrame, pose_of
        pk = lk = None
        self.points = self.lines = None
        if points_inp is not None:
            points_inp = own_copy(points_inp) if smash_sources else points_inp
            pk, self.points = PS.views(points_inp)
        if lines_inp is not None:
            lines_inp = own_copy(lines_inp) if smash_sources else lines_inp
            lk, self.lines = LS.views(lines_inp)
        K = len(pk if pk is not None else lk)
        assert pk is None or lk is None or len(pk) == len(lk)
        if pk is not None and lk is not None:   # one pose for both kinds: the line key frame's translation and centre
            self.poses = [KeyFramePose(pk[k].q_cw, lk[k].Rcw, lk[k].tcw, lk[k].Ow) for k in range(K)]
        else:
            self.poses = [pose_of(None if pk is None else pk[k], None if lk is None else lk[k]) for k in range(K)]
        self.kfs = [ResidentKeyFrame(None if pk is None else pk[k], None if lk is None else lk[k], host_only=host_only) for k in range(K)]
        if smash_sources:
            if points_inp is not None:
                smash(points_inp, POINT_ARRAYS)
            if lines_inp is not None:
                smash(lines_inp, LINE_ARRAYS)
            del pk, lk

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for kf in self.kfs:
            kf.close()


def search_points(inp, host, host_only=None, smash_sources=False, **kw):
    from plvs_amd.keyframe import fuse_search_kf
    with Handles(points_inp=inp, host_only=host if host_only is None else host_only, smash_sources=smash_sources) as h:
        return fuse_search_kf(h.kfs, h.poses, h.points, inp["th"], inp["skip"], host=host, **kw)


def search_lines(inp, host, host_only=None, smash_sources=False, **kw):
    from plvs_amd.keyframe import line_fuse_search_kf
    with Handles(lines_inp=inp, host_only=host if host_only is None else host_only, smash_sources=smash_sources) as h:
        return line_fuse_search_kf(h.kfs, h.poses, h.lines, inp["th"], inp["skip"], host=host, **kw)


def point_golden(path):
    from tests import orb_fuse_restatement as R
    return _golden(path, R.CANDIDATE)


def line_golden(path):
    from tests import line_fuse_restatement as R
    return _golden(path, R.CANDIDATE)


def _golden(path, candidate):
    g = dict(np.load(path))
    for pre in ("", "crowd_"):      # the entries' outputs from the recorded bestIdx / bestDist
        cand = g[pre + "reached"] == candidate
        g[pre + "best_idx"] = np.where(cand, g[pre + "raw_best_idx"], -1).astype(np.int32)
        g[pre + "best_dist"] = np.where(cand, g[pre + "raw_best_dist"], -1).astype(np.int32)
    return g


class ReplaySearcher:
    """search(kfs, items, skip) of tests/orb_fuse_replay.py / tests/line_fuse_replay.py over handles: one handle per key frame
    dictionary, made on first sight and kept (the replay re-queries single key frames of the batch's list)."""

    def __init__(self, kind, host):
        self.kind, self.host, self.made = kind, host, {}

    def __call__(self, kfs, items, skip):
        from plvs_amd.keyframe import ResidentKeyFrame, fuse_search_kf, line_fuse_search_kf, pose_of
        S = PS if self.kind == "points" else LS
        views, packed = S.views({"kfs": kfs, self.kind: items})
        hs, poses = [], []
        for kf, v in zip(kfs, views):
            if id(kf) not in self.made:
                self.made[id(kf)] = ResidentKeyFrame(**{self.kind: v}, host_only=self.host)
            hs.append(self.made[id(kf)])
            poses.append(pose_of(**{self.kind: v}))
        f = fuse_search_kf if self.kind == "points" else line_fuse_search_kf
        return f(hs, poses, packed, S.TH, skip, host=self.host)["best_idx"]

    def close(self):
        for h in self.made.values():
            h.close()
