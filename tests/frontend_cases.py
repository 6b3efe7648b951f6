"""The front-end geometry cases: images and settings at which the ORB and line kernels take another path than on the
640x480 / 1241x376 goldens — the sizes and settings the reference ships in its settings files, the smallest shapes that
reach the FAST cell and 64x16 tile edges, saturated / low-contrast / flat contents.  Run twice over the SAME table:
  tests/test_oracle_pinned_frontend.py, CPU   oracle/orb.cpp, oracle/lines.cpp equal the compiled reference on every case
  tests/test_frontend_geometry.py, GPU        the HIP path equals the oracle on every case, stage by stage
Every image is cut from a committed golden (or drawn from a seeded generator); nothing here reads a new fixture.

A case carries a floor — the least the ORACLE must produce before anything is compared, so that no case passes by
comparing nothing.  Each floor is about 90 % of what oracle/orb.cpp / oracle/lines.cpp (equal to the compiled reference,
see the CPU pin) gives on the case; the measured figure stands beside it.  `check_orb_floor` / `check_lines_floor`
assert them; they never look at the HIP output."""
import functools
from collections import namedtuple

import numpy as np

from tests.oracle_lib import golden
from tests.test_orb import synth_frame

_GOLDEN = {"aloe": "aloe_640x480.pgm", "cones": "cones_640x480.pgm", "urban1": "urban1_1241x376.pgm"}


def fit(img, w, h):
    """reflect-pad right / bottom where the golden is smaller, then crop to w x h"""
    ph, pw = max(0, h - img.shape[0]), max(0, w - img.shape[1])
    if ph or pw:
        img = np.pad(img, ((0, ph), (0, pw)), mode="reflect")
    return np.ascontiguousarray(img[:h, :w])


@functools.lru_cache(maxsize=None)
def image(name):
    """'<source>_<w>x<h>': aloe / cones / urban1 = fit(golden), edge = cones[100:, 200:] cropped, synth3 = synth_frame(3) drawn
    at that size, noise = uniform noise of default_rng(5), low / dim = fit(aloe) // 3 + 100 and // 8 + 100 (contrast 1/3 and
    1/8), flat = constant 93.  Read-only: shared between the tests."""
    src, size = name.split("_")
    w, h = (int(v) for v in size.split("x"))
    if src in _GOLDEN:
        img = fit(golden(_GOLDEN[src]), w, h)
    elif src == "edge":
        img = np.ascontiguousarray(golden(_GOLDEN["cones"])[100:100 + h, 200:200 + w])
    elif src == "noise":
        img = np.random.default_rng(5).integers(0, 256, (h, w), dtype=np.uint8)
    elif src == "synth3":
        img = synth_frame(3, w, h)
    elif src in ("low", "dim"):
        img = (fit(golden(_GOLDEN["aloe"]), w, h) // (3 if src == "low" else 8) + 100).astype(np.uint8)
    elif src == "flat":
        img = np.full((h, w), 93, np.uint8)
    else:
        raise KeyError(name)
    assert img.shape == (h, w) and img.dtype == np.uint8
    img.setflags(write=False)
    return img


# ------------------------------------------------------------------ ORB
# (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
DEFAULT = (1000, 1.2, 8, 20, 7)
SHIPPED = [DEFAULT, (1250, 1.2, 8, 20, 7), (1500, 1.2, 8, 15, 7), (500, 1.2, 8, 12, 7), (2000, 1.2, 8, 20, 7)]
SMALL_PYRAMIDS = [(300, 1.3, 4, 20, 7), (100, 1.5, 3, 15, 5), (200, 1.2, 1, 20, 7)]

# measured: (key points, pyramid levels that hold some) of the oracle on the case.  The floors follow from it: at least
# 90 % of the key points, and as many populated levels.
# rule: what the candidates of all levels must say about the per-cell rule "iniThFAST, else minThFAST" —
#   "both"  responses >= iniThFAST and < iniThFAST both occur: some cells pass the first threshold, others fall back
#   "below" candidates exist and every one is < iniThFAST: every cell falls back
OrbCase = namedtuple("OrbCase", "id image settings measured rule")


def _orb(image_name, settings, kps, levels, rule=None):
    return OrbCase(image_name + "-" + "-".join(str(v) for v in settings), image_name, settings, (kps, levels), rule)


def _edge(size, *measured):
    """an edge size under the default and the three small pyramids"""
    return [_orb("edge_" + size, st, *m) for st, m in zip([DEFAULT] + SMALL_PYRAMIDS, measured)]


ORB_CASES = [
    # full sizes of the shipped settings files (EuRoC 752x480, TUM-VI 512x512, RealSense 848x480 / 848x800, 1280x720,
    # 672x360, KITTI 1226x370): the default and one other shipped setting each
    _orb("aloe_752x480", DEFAULT, 1014, 8), _orb("aloe_752x480", SHIPPED[1], 1260, 8),
    _orb("cones_512x512", DEFAULT, 1008, 8), _orb("cones_512x512", SHIPPED[2], 1507, 8),
    _orb("aloe_848x480", DEFAULT, 1012, 8), _orb("aloe_848x480", SHIPPED[3], 511, 8),
    _orb("cones_848x800", DEFAULT, 1005, 8), _orb("cones_848x800", SHIPPED[4], 2010, 8),
    _orb("aloe_1280x720", DEFAULT, 1012, 8), _orb("aloe_1280x720", SHIPPED[1], 1256, 8),
    _orb("urban1_672x360", DEFAULT, 1005, 8), _orb("urban1_672x360", SHIPPED[2], 1504, 8),
    _orb("urban1_1226x370", DEFAULT, 1005, 8), _orb("urban1_1226x370", SHIPPED[4], 2006, 8),
    # cell edges.  A level's cell region is w - 32 wide and holds (w - 32) / 35 columns: none below 67 px ...
    *_edge("66x66", (0, 0), (0, 0), (0, 0), (0, 0)),              # ... so nothing at all, on either side
    *_edge("67x67", (22, 1), (22, 1), (32, 1), (22, 1)),          # the first level with one cell
    *_edge("101x101", (151, 3), (122, 2), (79, 2), (85, 1)),      # one cell of the maximal 69-px window ...
    *_edge("102x102", (169, 3), (128, 2), (79, 2), (91, 1)),      # ... against two columns and two rows
    *_edge("101x67", (35, 1), (35, 1), (47, 1), (35, 1)),         # each axis alone
    *_edge("67x102", (48, 1), (48, 1), (47, 1), (48, 1)),
    *_edge("136x137", (474, 4), (243, 3), (82, 2), (200, 1)),     # 104 / 105 px of cells: 2 columns of 52, 3 rows of 35
    *_edge("137x136", (487, 4), (244, 3), (79, 2), (200, 1)),
    # tile edges of fast_score_map / blur_levels (64x16): level 0 is k*64+1 wide and k*16+1 high ...
    *_edge("129x81", (143, 2), (90, 1), (47, 1), (90, 1)),
    # ... and a level of exactly 2x5 tiles whose pitch equals its width: level 1 of 154x96 at 1.2 is 128x80 (a level that
    # is 64 wide itself has no cell: 77x77 -> 64x64)
    *_edge("154x96", (276, 3), (175, 2), (47, 1), (142, 1)),
    _orb("edge_77x77", DEFAULT, 29, 1),
    _orb("edge_333x181", SMALL_PYRAMIDS[0], 304, 4),              # all four levels of the 1.3 pyramid populated
    # contents.  Uniform noise saturates every cell (5883 level-0 candidates): nfeatures far below, near and far above what
    # the quadtree is offered
    _orb("noise_320x240", (50, 1.2, 8, 20, 7), 71, 8), _orb("noise_320x240", DEFAULT, 958, 8),
    _orb("noise_320x240", (5000, 1.2, 8, 20, 7), 4206, 8),
    # contrast 1/3: at each of the shipped threshold pairs some cells pass iniThFAST and the others fall back
    _orb("low_752x480", (1000, 1.2, 8, 20, 7), 1007, 8, "both"), _orb("low_752x480", (1000, 1.2, 8, 15, 5), 1004, 8, "both"),
    _orb("low_752x480", (1000, 1.2, 8, 12, 4), 1004, 8, "both"),
    # contrast 1/8: no response reaches iniThFAST, every cell falls back to minThFAST
    _orb("dim_752x480", (1000, 1.2, 8, 20, 7), 286, 4, "below"), _orb("dim_752x480", (1000, 1.2, 8, 15, 5), 682, 8, "below"),
    _orb("dim_752x480", (1000, 1.2, 8, 12, 4), 919, 8, "below"),
    _orb("flat_320x240", DEFAULT, 0, 0),
]
assert len({c.id for c in ORB_CASES}) == len(ORB_CASES)


def orb_case(image_name, settings=DEFAULT):
    return next(c for c in ORB_CASES if c.image == image_name and c.settings == settings)


def scale_tables(settings):
    """(mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2) of ORBextractor.cc:455-470: float tables, the
    recurrence through the double member scaleFactor.  The CPU pin holds the compiled reference to this statement."""
    _, sf, nl, _, _ = settings
    s = [np.float32(1)]
    for _ in range(1, nl):
        s.append(np.float32(np.float64(s[-1]) * np.float64(np.float32(sf))))
    s = np.array(s, np.float32)
    s2 = (s * s).astype(np.float32)
    return s, (np.float32(1) / s).astype(np.float32), s2, (np.float32(1) / s2).astype(np.float32)


OrbResult = namedtuple("OrbResult", "mono kps desc levels blurred candidates features_per_level")
_orb_results = {}


def oracle_orb(oracle, case, lap=(0, 0)):
    """The oracle's result of a case, every stage of it, computed once and shared (read-only) between the tests."""
    key = (case.id, lap)
    if key not in _orb_results:
        nl = case.settings[2]
        e = oracle.orb(*case.settings)
        mono, kps, desc = e.extract(image(case.image), lap)
        blurred = [e.level(k, True) if np.any(kps["octave"] == k) else None   # (a level without key points is not blurred)
                   for k in range(nl)]
        r = OrbResult(mono, kps, desc, [e.level(k) for k in range(nl)], blurred, [e.candidates(k) for k in range(nl)],
                      e.features_per_level())
        for a in (r.kps, r.desc, r.features_per_level, *r.levels, *r.candidates, *[b for b in r.blurred if b is not None]):
            a.setflags(write=False)
        _orb_results[key] = r
    return _orb_results[key]


def check_orb_floor(case, r):
    """the oracle's output `r` of `case` is not vacuous"""
    kps, levels = case.measured
    assert len(r.kps) * 10 >= kps * 9, f"{case.id}: {len(r.kps)} key points, measured {kps}"
    assert len(np.unique(r.kps["octave"])) >= levels, f"{case.id}: levels {np.unique(r.kps['octave'])}, measured {levels}"
    if kps == 0:
        assert len(r.kps) == 0 and all(len(c) == 0 for c in r.candidates), f"{case.id}: expected nothing"
    if case.rule:
        resp = np.concatenate([c[:, 2] for c in r.candidates])
        ini = case.settings[3]
        assert (resp < ini).any(), f"{case.id}: no candidate below iniThFAST"
        assert (resp >= ini).any() == (case.rule == "both"), f"{case.id}: {int((resp >= ini).sum())} candidates >= iniThFAST"


# ------------------------------------------------------------------ lines
LINE_DEFAULT = dict(nfeatures=100, nlevels=3, scale=1.2, min_length=0.02, fit_err=1.6)
LINE_SETTINGS = {"default": LINE_DEFAULT,
                 "one": dict(LINE_DEFAULT, nfeatures=50, nlevels=1),                       # Line.nLevels: 1
                 "long": dict(LINE_DEFAULT, nfeatures=200, min_length=0.1, fit_err=1.0),
                 "four": dict(LINE_DEFAULT, nlevels=4, scale=1.5, fit_err=2.5)}

# measured: KeyLines of the oracle on the case; the floor is 90 % of it
LineCase = namedtuple("LineCase", "id image setting measured")


def _lines(image_name, setting, measured):
    return LineCase(f"{image_name}-{setting}", image_name, setting, measured)


# "long" keeps lines of at least a tenth of the image's longer side: aloe and cones have (next to) none, at any of these
# sizes, so it runs on the synthetic rectangles (and on urban1 at 1280x720); at 333x181 no source gives it a line, it is left
# out there
LINE_CASES = [
    _lines("aloe_752x480", "default", 100), _lines("aloe_752x480", "four", 100), _lines("synth3_752x480", "long", 80),
    _lines("cones_512x512", "default", 100), _lines("cones_512x512", "one", 50), _lines("synth3_512x512", "long", 138),
    _lines("aloe_1280x720", "default", 100), _lines("aloe_1280x720", "four", 100), _lines("urban1_1280x720", "long", 56),
    _lines("aloe_333x181", "default", 100), _lines("aloe_333x181", "one", 50), _lines("aloe_333x181", "four", 100),
    _lines("aloe_127x97", "default", 25), _lines("aloe_127x97", "one", 17), _lines("aloe_127x97", "four", 25),
    _lines("synth3_127x97", "long", 13),
    _lines("aloe_101x67", "default", 17), _lines("aloe_101x67", "one", 12), _lines("aloe_101x67", "four", 16),
    _lines("synth3_101x67", "long", 7),
    _lines("aloe_64x48", "default", 7), _lines("aloe_64x48", "one", 6), _lines("aloe_64x48", "four", 11),
    _lines("synth3_64x48", "long", 5),
]
assert len({c.id for c in LINE_CASES}) == len(LINE_CASES)


def line_case(image_name, setting="default"):
    return next(c for c in LINE_CASES if c.image == image_name and c.setting == setting)


def check_lines_floor(case, keylines):
    assert len(keylines) * 10 >= case.measured * 9, f"{case.id}: {len(keylines)} lines, measured {case.measured}"
