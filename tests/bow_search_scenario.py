"""The scenario of ORBmatcher::SearchByBoW over resident key frames (tests/test_bow_search.py, scripts/make_bow_search_golden.py): two
"A" objects — A0, a key frame / frame of ~240 key points under 16 vocabulary nodes, and A1, the degenerate vocabulary (200 key
points under ONE node) — and K = 12 key frames B[k].  The key-frame kind runs SearchByBoW(A, B[k]) (A serial, B[k] on lanes), the
frame kind SearchByBoW(B[k], F = A) (B[k] serial, A on lanes).  Descriptors are crafted to exact Hamming distances: a member is its
query with chosen bits flipped; unrelated descriptors are random (about 128 bits apart).  What the reference does at every placed
case is recorded in tests/golden/bow_search_reference_facts.json and asserted from there.

A side: dict(desc [n,32] u8, angle [n] f32, ref_valid [n] u8 (0: no map point, 1: good, 2: isBad()), nodes {node id: [features in
list order]}).  valid = ref_valid == 1 is what the library is given.  scenario() -> (sides, where): where[name] = dict(kind, k, node,
queries (serial-side features), members (lane-side features)) of every placed case."""
import hashlib

import numpy as np

K = 12
RUNS = (("r075_ori", 0.75, 1), ("r15_plain", 1.5, 0), ("r09_ori", 0.9, 1))   # (name, nn_ratio, check_orientation)
KF, FRAME = "kf", "frame"
DEGENERATE_NODE = 777


class _Side:
    def __init__(self):
        self.desc, self.angle, self.ref_valid, self.nodes, self.node_of = [], [], [], {}, []

    def add(self, node, desc, angle=0.0, ref_valid=1, front=False):
        i = len(self.desc)
        self.desc.append(desc)
        self.angle.append(angle)
        self.ref_valid.append(ref_valid)
        self.node_of.append(node)
        if node is not None:
            lst = self.nodes.setdefault(node, [])
            lst.insert(0, i) if front else lst.append(i)
        return i

    def done(self):
        n = len(self.desc)
        return dict(desc=np.array(self.desc, np.uint8).reshape(n, 32), angle=np.array(self.angle, np.float32),
                    ref_valid=np.array(self.ref_valid, np.uint8), nodes={k: list(v) for k, v in sorted(self.nodes.items())})


def flip(desc, bits):
    """desc with exactly these bit positions flipped: Hamming distance len(bits)."""
    out = np.array(desc, np.uint8).copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def valid_of(side):
    return (side["ref_valid"] == 1).astype(np.uint8)


def build():
    rng = np.random.default_rng(20261021)
    rand = lambda: rng.integers(0, 256, 32, dtype=np.uint8)
    near = lambda d, bits: flip(d, rng.choice(256, bits, replace=False))
    A0, A1 = _Side(), _Side()
    B = [_Side() for _ in range(K)]
    where = {}
    # the rotation a generic match gets: most in bin 0, some in 3 and 5, a few (cut) in 7
    rot_of = lambda: float(rng.choice([0.0, 90.0, 150.0, 210.0], p=[0.6, 0.15, 0.15, 0.1]) + rng.uniform(-8, 8))

    def generic(node, ks, n_a, n_b, match_frac=0.6, invalid_frac=0.1):
        """n_a features of A0 under `node`; every B[k], k in ks, gets n_b[k] members: near copies (5..45 bits) of some A features, the rest random."""
        a_idx = [A0.add(node, rand(), float(rng.uniform(0, 360)), 1 if rng.random() > invalid_frac else int(rng.choice([0, 2])))
                 for _ in range(n_a)]
        for k, nb in zip(ks, n_b):
            for j in range(nb):
                v = 1 if rng.random() > invalid_frac else int(rng.choice([0, 2]))
                if rng.random() < match_frac:
                    src = a_idx[int(rng.integers(0, n_a))]
                    ang = (A0.angle[src] - rot_of()) % 360.0
                    B[k].add(node, near(A0.desc[src], int(rng.integers(5, 46))), ang, v)
                else:
                    B[k].add(node, rand(), float(rng.uniform(0, 360)), v)
        return a_idx

    # ---- nodes present on one side only: front, middle, end of the id lists
    A0.add(2, rand())                       # A-only, front
    for k in range(K):
        if k != 9:
            B[k].add(1, rand())             # B-only, front
            B[k].add(455, rand())           # B-only, middle
            B[k].add(9999, rand())          # B-only, end
    A0.add(450, rand())                     # A-only, middle
    A0.add(9000, rand())                    # A-only, end (below B's 9999: the walk ends on A's side first)
    # ---- the list lengths.  Key-frame kind: the claimed side is B[k]; frame kind: A0
    generic(10, [0, 1], 1, [1, 2], invalid_frac=0.0)                  # A len 1 (a querying list of 1 in the kf kind; a claimed list of 1 in the frame kind)
    generic(20, [0, 1, 2], 2, [63, 64, 1], invalid_frac=0.0)   # A len 2; B lens 63, 64 (kf kind); k = 2: a querying list of 1 in the frame kind
    generic(30, [2, 3], 5, [65, 129])               # B lens 65, 129: more than one pass
    generic(40, [3, 4], 63, [3, 70])                # A lens 63, 64, 65: the frame kind's claimed lists
    generic(50, [4, 5], 64, [4, 5])
    generic(60, [5, 6], 65, [66, 7])
    # ---- crafted cases: a query q and members at exact distances.  kind = KF: q in A0, members in B[k]; FRAME: q in B[k], members in A0
    # Node ids are shared where that changes nothing: the kf kind's queries of different k sit under nodes 100 / 103 of A0 (a query sees
    # only its own k's members); the frame kind's members of different k sit under node 110 of A0 (a query sees the other cases' members
    # too, about 128 bits away), except the two cases that need the list to themselves (nodes 113, 116).
    def craft(name, kind, k, node, dists, q_angle=100.0, m_angles=None, m_valid=None, order=None, n_queries=1, q_bits=()):
        S, L = (A0, B[k]) if kind == KF else (B[k], A0)
        assert kind == FRAME or node not in B[k].nodes, "two kf-kind cases under one (k, node)"
        assert kind == KF or node not in B[k].nodes, "two frame-kind cases under one (k, node)"
        q = rand()
        qs = [S.add(node, q if i == 0 else flip(q, q_bits[i - 1]), q_angle) for i in range(n_queries)]
        ms = []
        for j, d in enumerate(dists):
            bits = d if not isinstance(d, int) else range(16 + 64 * j, 16 + 64 * j + d)
            ms.append(L.add(None, flip(q, list(bits)), 100.0 if m_angles is None else m_angles[j], 1 if m_valid is None else m_valid[j]))
        L.nodes.setdefault(node, []).extend(ms[j] for j in (order or range(len(ms))))
        where[name + "_" + kind] = dict(kind=kind, k=k, node=node, queries=qs, members=ms)

    cases = [
        ("single_member", dict(dists=[20])),                                         # bestDist2 stays 256
        ("equal_minima", dict(dists=[30, 30])),                                      # the earlier position wins; ratio fails below 1, passes at 1.5
        ("tie_descending", dict(dists=[30, 30], order=[1, 0])),                      # the list in descending index order: the winner is the HIGHER index
        # the best is claimed by the first query, the second query takes the runner-up: q2 = q1 with bits 200, 201 flipped
        ("second_taken", dict(dists=[list(range(0, 5)), list(range(10, 35))], n_queries=2, q_bits=[[200, 201]])),
        # every member claimed or invalid: the second query finds nothing open (the frame kind has no validity gate on its lane side)
        ("all_closed", None),
        ("at_49", dict(dists=[49])),
        ("at_50", dict(dists=[50])),                                                 # the frame kind accepts, the key-frame kind rejects
        ("at_51", dict(dists=[51])),
        ("ratio_equal", dict(dists=[list(range(0, 30)), list(range(100, 140))])),    # 30 == 0.75f * 40 exactly: rejected at 0.75, taken at 0.9
        # kp.angle - other.angle = -10 -> 350 -> 11.67 -> bin 12 -> 0 (kf kind: A - B; frame kind: KF - F = B - A)
        ("bin_12", dict(dists=[10], q_angle=20.0, m_angles=[30.0])),
    ]
    for i, (name, kw) in enumerate(cases):
        if name == "all_closed":
            craft(name, KF, 4 + i // 2, 100 + 3 * (i % 2), [list(range(0, 6)), list(range(10, 20))], n_queries=2, q_bits=[[200, 201]], m_valid=[1, 2])
            craft(name, FRAME, 7, 116, [list(range(0, 6))], n_queries=2, q_bits=[[200, 201]])
            continue
        craft(name, KF, 4 + i // 2, 100 + 3 * (i % 2), **kw)
        if name == "single_member":
            craft(name, FRAME, 6, 113, **kw)
        else:
            craft(name, FRAME, i - 1 if i < 4 else i - 2, 110, **kw)
    # ---- a bin tie in ComputeThreeMaxima: B[10] holds nine matches under one node, and nothing else in common, rotations 3 x 0, 2 x 60, 2 x 120, 2 x 180 degrees:
    # bins 0, 2, 4 survive and bin 6 loses the tie with bin 4 (s > max3 is strict); the frame kind sees 0, 10, 8, 6 and keeps 0, 6, 8
    for j, rot in enumerate([0, 0, 0, 60, 60, 120, 120, 180, 180]):
        q = rand()
        node = 500
        a = A0.add(node, q, 200.0)
        B[10].add(node, near(q, 10), 200.0 - rot)
        if j == 0:
            where["bin_tie"] = dict(kind="both", k=10, node=node, queries=[a], members=[])
    # ---- k = 9: no common node with A0 (and none of the one-sided nodes above); k = 11: valid all zero;  B[9] keeps one node A lacks
    B[9].add(7, rand())
    where["no_common_node"] = dict(kind="both", k=9, node=7, queries=[], members=[])
    generic(70, [11], 4, [6])
    where["all_invalid"] = dict(kind="both", k=11, node=70, queries=[], members=[])
    # ---- the degenerate vocabulary: every feature of A1 and of its partner under one node, ~200 each
    a1 = [A1.add(DEGENERATE_NODE, rand(), float(rng.uniform(0, 360)), 1 if rng.random() > 0.1 else int(rng.choice([0, 2]))) for _ in range(200)]
    Bd = [_Side() for _ in range(K)]
    for j in range(200):
        v = 1 if rng.random() > 0.1 else int(rng.choice([0, 2]))
        if rng.random() < 0.6:
            src = a1[int(rng.integers(0, 200))]
            Bd[0].add(DEGENERATE_NODE, near(A1.desc[src], int(rng.integers(5, 46))), (A1.angle[src] - rot_of()) % 360.0, v)
        else:
            Bd[0].add(DEGENERATE_NODE, rand(), float(rng.uniform(0, 360)), v)
    sides = dict(A0=A0.done(), A1=A1.done(), B=[b.done() for b in B], Bd=Bd[0].done())
    sides["B"][11]["ref_valid"][:] = 0
    empty = _Side()
    empty.add(None, rand())                      # a key frame with one key point and an empty vector
    sides["empty"] = empty.done()
    for s in [sides["A0"], sides["A1"], sides["Bd"], sides["empty"]] + sides["B"]:
        assert len(s["desc"]) <= 300, len(s["desc"])
        listed = [i for v in s["nodes"].values() for i in v]
        assert len(listed) == len(set(listed)), "a feature under two nodes"
        assert len(s["nodes"]) <= 24
    return sides, where


_CACHE = None


def scenario():
    global _CACHE
    if _CACHE is None:
        _CACHE = build()
    return _CACHE


def calls():
    """The calls of the scenario: name -> (A side, [B sides]).  `main`: A0 against the 12 key frames; `degenerate`: A1 against its
    partner, a key frame with an empty vector, A0's first key frame (no common node) and the partner once more."""
    s, _ = scenario()
    return dict(main=(s["A0"], s["B"]), degenerate=(s["A1"], [s["Bd"], s["empty"], s["B"][0], s["Bd"]]))


def random_sides(seed, n_a, n_b, n_kfs, n_nodes, match_frac=0.5):
    """An unstructured set at another size: every feature under a random node, B's partly near copies of A's (same node)."""
    rng = np.random.default_rng(seed)

    def side(n, src=None):
        s = _Side()
        for i in range(n):
            v = 1 if rng.random() > 0.15 else int(rng.choice([0, 2]))
            if src is not None and rng.random() < match_frac and len(src.desc):
                j = int(rng.integers(0, len(src.desc)))
                node = src.node_of[j]
                s.add(node, flip(src.desc[j], rng.choice(256, int(rng.integers(0, 70)), replace=False)), float(rng.uniform(0, 360)), v)
            else:
                s.add(int(rng.integers(0, n_nodes)) * 3, rng.integers(0, 256, 32, dtype=np.uint8), float(rng.uniform(0, 360)), v)
        return s

    A = side(n_a)
    Bs = [side(n_b, A).done() for _ in range(n_kfs)]
    for b in Bs:                                   # list order is not index order
        for lst in b["nodes"].values():
            rng.shuffle(lst)
    return A.done(), Bs


def digest(side):
    h = hashlib.sha256()
    for k in ("desc", "angle", "ref_valid"):
        h.update(np.ascontiguousarray(side[k]).tobytes())
    for node, lst in sorted(side["nodes"].items()):
        h.update(np.array([node, len(lst)] + list(lst), np.int64).tobytes())
    return h.hexdigest()


def digests():
    s, _ = scenario()
    out = dict(A0=digest(s["A0"]), A1=digest(s["A1"]), Bd=digest(s["Bd"]), empty=digest(s["empty"]))
    out.update({f"B{k}": digest(b) for k, b in enumerate(s["B"])})
    return out


def nominal(kind_k=33, n=1500, n_nodes=100, seed=11):
    """The measurement's shape (scripts/measure_bow_search.py, make_bow_search_golden.py --time): one side of n key points against kind_k
    key frames of n, about n_nodes vocabulary nodes."""
    return random_sides(seed, n, n, kind_k, n_nodes)


# ---- the library's objects of a side (imported late: the scenario itself needs numpy alone)
def feature_vector(side):
    from plvs_amd.orbmatcher import FeatureVector
    return FeatureVector({k: list(v) for k, v in side["nodes"].items()})


def point_side(side):
    """A FuseKeyFrame around the side's descriptors: SearchByBoW reads nothing else of the point side, so the key points sit on a lattice."""
    from plvs_amd.orbmatcher import FrameView, FuseKeyFrame
    n = len(side["desc"])
    i = np.arange(n)
    view = FrameView(x=(10.0 + 37.0 * (i % 16)).astype(np.float32), y=(10.0 + 23.0 * (i // 16)).astype(np.float32), octave=np.zeros(n, np.int32),
                     u_right=np.full(n, -1.0, np.float32), desc=side["desc"], min_x=0.0, min_y=0.0, grid_w_inv=64 / 640.0, grid_h_inv=48 / 480.0,
                     scale_factors=np.array([1.0, 1.2], np.float32))
    return FuseKeyFrame(view=view, inv_level_sigma2=np.array([1.0, 1 / 1.44], np.float32), log_scale_factor=float(np.log(1.2)),
                        K4=np.array([500, 500, 320, 240], np.float32), mbf=40.0, bounds4=np.array([0, 640, 0, 480], np.float32),
                        q_cw=np.zeros(4, np.float32), tcw=np.zeros(3, np.float32), Ow=np.zeros(3, np.float32))


def key_frame(side, host_only=False, vec=None, angle="side"):
    from plvs_amd.keyframe import KeyFrameBow, ResidentKeyFrame
    bow = KeyFrameBow(feature_vector(side) if vec is None else vec, side["angle"] if isinstance(angle, str) else angle)
    return ResidentKeyFrame(points=point_side(side), host_only=host_only, bow=bow)


def bow_frame(side, vec=None):
    from plvs_amd.keyframe import BowFrame
    return BowFrame(side["desc"], side["angle"], feature_vector(side) if vec is None else vec)
