"""Synthetic inputs for libelas' post-processing stages and for computeDisparity's triangle loop: named, seeded builders of
float32 disparity maps [H, W] (invalid pixels -10 unless a case says otherwise) at the exact thresholds, line ends and chunk
boundaries where a per-thread reformulation of the reference's serial code goes wrong.

Every case is a dict: `name`, `stage` ('seg' | 'gap' | 'mean' | 'lr' | 'tri'), the map(s), the parameters of the stage and
`facts`: {what the case must contain: how often it does}.  A test asserts every fact >= 1 (`assert_facts`), so a case cannot
silently stop exercising its edge.  `width` / `height` are the IMAGE size (twice the map's with subsampling, an odd one
where the halving must round).  Plain module: no fixtures, no GPU, no compiled reference."""
import numpy as np

INVALID = np.float32(-10.0)
ONE_UP = np.nextafter(np.float32(1), np.float32(2))        # the smallest difference that is no longer similar (threshold 1)
THREE_DOWN = np.nextafter(np.float32(3), np.float32(0))    # the largest difference gapInterpolation still averages over
SIM = 1.0                                                  # speckle_sim_threshold of both parameter sets (elas.h:117, :144)


def speckle_of(speckle_size, subsampling):
    """The segment size removeSmallSegments compares with (elas.cpp:1051)."""
    return int(np.float32(np.sqrt(np.float32(speckle_size))) * np.float32(2)) if subsampling else int(speckle_size)


def gap_of(ipol_gap_width, subsampling):
    """The gap width gapInterpolation compares with (elas.cpp:1172)."""
    return ipol_gap_width // 2 + 1 if subsampling else ipol_gap_width


def image_size(shape, subsampling, odd=False):
    """(width, height) of an image whose disparity map has `shape`; odd: one that the halving rounds down."""
    h, w = shape
    return (2 * w + int(odd), 2 * h + int(odd)) if subsampling else (w, h)


def assert_facts(case):
    missing = {k: v for k, v in case["facts"].items() if int(v) < 1}
    assert not missing, f"{case['name']}: the case no longer holds {missing}"


# ------------------------------------------------------------------ the connected-component model of the device path
def components(D, sim=SIM):
    """4-connected components of the relation 'both valid and |a - b| <= sim' -> (root index per pixel [H, W], size per
    root [H * W]; invalid pixels are components of their own with size 0)."""
    D = np.asarray(D, np.float32)
    H, W = D.shape
    parent = list(range(H * W))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    valid = D >= 0
    with np.errstate(invalid="ignore"):
        right = valid[:, :-1] & valid[:, 1:] & (np.abs(D[:, :-1] - D[:, 1:]) <= np.float32(sim))
        down = valid[:-1, :] & valid[1:, :] & (np.abs(D[:-1, :] - D[1:, :]) <= np.float32(sim))
    for (mask, step) in ((right, 1), (down, W)):
        for v, u in zip(*np.nonzero(mask)):
            a, b = find(int(v) * W + int(u)), find(int(v) * W + int(u) + step)
            if a != b:
                parent[max(a, b)] = min(a, b)
    roots = np.array([find(i) for i in range(H * W)], np.int64).reshape(H, W)
    sizes = np.bincount(roots[valid], minlength=H * W)
    return roots, sizes


def component_model(D, speckle, sim=SIM):
    """What the device's union-find computes: components smaller than `speckle` (an invalid pixel counts as one of size 1)
    go to -10.  Equal to Elas::removeSmallSegments where every invalid pixel holds -10 and sim < 10."""
    D = np.asarray(D, np.float32)
    roots, sizes = components(D, sim)
    out = D.copy()
    valid = D >= 0
    out[valid & (sizes[roots] < speckle)] = INVALID
    if 1 < speckle:
        out[~valid] = INVALID
    return out


def _size_histogram(D, sim=SIM):
    roots, sizes = components(D, sim)
    return np.bincount(sizes[sizes > 0])


class _Canvas:
    """Patches side by side, one invalid pixel between them, wrapped into bands."""

    def __init__(self, W, H):
        self.D = np.full((H, W), INVALID, np.float32)
        self.x = self.y = self.band = 0

    def place(self, patch):
        h, w = patch.shape
        H, W = self.D.shape
        if self.x + w > W:
            self.x, self.y, self.band = 0, self.y + self.band + 1, 0
        assert w <= W and self.y + h <= H, f"canvas {W} x {H} too small"
        self.D[self.y:self.y + h, self.x:self.x + w] = patch
        self.x, self.band = self.x + w + 1, max(self.band, h)


def _blob(n, bw, value):
    """n pixels filled row-major into a box bw wide; value(row, col) -> disparity."""
    h = -(-n // bw)
    patch = np.full((h, bw), INVALID, np.float32)
    for i in range(n):
        patch[i // bw, i % bw] = value(i // bw, i % bw)
    return patch


def _seg_case(name, D, speckle_size, subsampling, facts):
    w, h = image_size(D.shape, subsampling)
    return dict(name=name, stage="seg", D=np.ascontiguousarray(D, np.float32), speckle_size=speckle_size, subsampling=bool(subsampling),
                width=w, height=h, facts=facts)


def _kept_removed(D, s):
    hist = _size_histogram(D)
    n = np.arange(len(hist))
    return {"segments the stage keeps": int(hist[n >= s].sum()), "segments the stage removes": int(hist[(n < s) & (n > 0)].sum())}


# ------------------------------------------------------------------ removeSmallSegments
def seg_sizes(W, H, speckle_size, subsampling, seed):
    """Isolated blobs of exactly s - 1, s and s + 1 pixels (twice each), disparities within the similarity threshold."""
    s = speckle_of(speckle_size, subsampling)
    rng = np.random.default_rng(seed)
    c = _Canvas(W, H)
    bw = min(W, int(np.sqrt(s)) + 3)
    for rep in range(2):
        for n in (s - 1, s, s + 1):
            base = np.float32(rng.integers(0, 40))
            c.place(_blob(n, bw, lambda r, k: base + np.float32(rng.integers(0, 3)) * np.float32(0.25)))
    hist = _size_histogram(c.D)
    facts = {f"segments of {n} pixels (speckle size {s})": int(hist[n]) if n < len(hist) else 0 for n in (s - 1, s, s + 1)}
    return _seg_case(f"seg_sizes_{W}x{H}_size{speckle_size}_sub{int(subsampling)}", c.D, speckle_size, subsampling, facts)


def seg_threshold(W, H, speckle_size, subsampling):
    """Blobs of exactly s pixels in two halves whose disparities differ by exactly the threshold (one segment: kept) or by
    the next float (two segments: removed); ramps 0, 1, 2 ... (similarity is not transitive); fractions and -0.0."""
    s = speckle_of(speckle_size, subsampling)
    c = _Canvas(W, H)
    bw = min(W, int(np.sqrt(s)) + 3)
    halves = [(0.0, 1.0), (0.0, ONE_UP), (-0.0, 1.0), (0.25, 1.25), (0.5, np.nextafter(np.float32(1.5), np.float32(2))), (7.5, 6.5),
              (3.0, 3.0 + 1.5)]
    for a, b in halves:
        c.place(_blob(s, bw, lambda r, k, a=a, b=b: np.float32(a) if k < bw // 2 else np.float32(b)))
    c.place(_blob(s, bw, lambda r, k: np.float32(k)))                       # a ramp of step 1: one segment
    c.place(_blob(s, bw, lambda r, k: np.float32(k) * np.float32(1.5)))     # a ramp of step 1.5: columns apart
    D = c.D
    valid_h = (D[:, :-1] >= 0) & (D[:, 1:] >= 0)
    diff_h = np.abs(D[:, :-1] - D[:, 1:])
    facts = {"neighbours that differ by exactly 1.0": int((valid_h & (diff_h == np.float32(1))).sum()),
             "neighbours that differ by nextafter(1.0, 2)": int((valid_h & (diff_h == ONE_UP)).sum()),
             "pixels at -0.0": int(((D == 0) & np.signbit(D)).sum()),
             "fractional disparities": int(((D >= 0) & (D != np.floor(D))).sum())}
    facts.update(_kept_removed(D, s))
    roots, sizes = components(D)
    far = 0          # pixels of one segment that are not similar to each other
    for root in np.unique(roots[D >= 0]):
        vals = D[(roots == root) & (D >= 0)]
        far += int(vals.max() - vals.min() > SIM)
    facts["segments that hold pixels not similar to each other"] = far
    return _seg_case(f"seg_threshold_{W}x{H}_size{speckle_size}_sub{int(subsampling)}", D, speckle_size, subsampling, facts)


def _one_segment_facts(D, s, widest_run):
    hist = _size_histogram(D)
    n = np.arange(len(hist))
    return {"one segment in all": int(hist.sum() == 1), "kept as a whole": int(hist[n >= s].sum() == 1),
            "removed if it fell apart into its runs": int(widest_run < s)}


def seg_comb(W, H, speckle_size, subsampling, last_column=True):
    """Teeth (every other row, full width) that meet only in the last (or first) column."""
    D = np.full((H, W), INVALID, np.float32)
    D[0::2, :] = 3.0
    D[:, W - 1 if last_column else 0] = 3.0
    return _seg_case(f"seg_comb_{'last' if last_column else 'first'}_{W}x{H}_sub{int(subsampling)}", D, speckle_size, subsampling,
                     _one_segment_facts(D, speckle_of(speckle_size, subsampling), W))


def seg_two_runs(W, speckle_size, subsampling, at_last, rows_reach_the_size=False):
    """Two rows, each one run, joined only by the vertical pair at u = 0 (or u = W - 1): the lower run climbs by 0.5 a pixel.
    rows_reach_the_size: a width at which either row alone is kept or both together are removed (no size fact then)."""
    D = np.empty((2, W), np.float32)
    D[0] = 3.0
    ramp = np.float32(4.0) + np.float32(0.5) * np.arange(W, dtype=np.float32)
    D[1] = ramp[::-1] if at_last else ramp
    with np.errstate(invalid="ignore"):
        joins = np.nonzero(np.abs(D[0] - D[1]) <= np.float32(SIM))[0]
    facts = _one_segment_facts(D, speckle_of(speckle_size, subsampling), W)
    if rows_reach_the_size:
        facts = {"one segment in all": facts["one segment in all"]}
    facts["joined by one vertical pair, at the line's end"] = int(len(joins) == 1 and joins[0] == (W - 1 if at_last else 0))
    return _seg_case(f"seg_two_runs_{'last' if at_last else 'first'}_{W}_sub{int(subsampling)}", D, speckle_size, subsampling, facts)


def seg_u_and_spiral(speckle_size, subsampling, size=25):
    """A U (two columns and the bottom row) and a one-pixel-wide square spiral."""
    U = np.full((size, size), INVALID, np.float32)
    U[:, 0] = U[:, -1] = U[-1, :] = 7.0
    S = np.full((size, size), INVALID, np.float32)
    inside = lambda y, x: 0 <= y < size and 0 <= x < size          # noqa: E731
    turns = ((0, 1), (1, 0), (0, -1), (-1, 0))
    y = x = heading = 0
    S[0, 0] = 9.0
    while True:      # straight on until the next pixel or the one behind it is taken, then one turn to the right
        for attempt in range(2):
            dy, dx = turns[heading]
            free = inside(y + dy, x + dx) and S[y + dy, x + dx] < 0 and not (inside(y + 2 * dy, x + 2 * dx) and S[y + 2 * dy, x + 2 * dx] >= 0)
            if free:
                break
            heading = (heading + 1) % 4
        if not free:
            break
        y, x = y + dy, x + dx
        S[y, x] = 9.0
    D = np.full((size, 2 * size + 1), INVALID, np.float32)
    D[:, :size], D[:, size + 1:] = U, S
    s = speckle_of(speckle_size, subsampling)
    hist = _size_histogram(D)
    n = np.arange(len(hist))
    facts = {"two segments (the U and the spiral)": int(hist.sum() == 2), "both kept": int(hist[n >= s].sum() == 2),
             "removed if they fell apart into their runs": int(size < s),
             "the spiral is one pixel wide": int(not ((S[:-1, :-1] >= 0) & (S[1:, :-1] >= 0) & (S[:-1, 1:] >= 0) & (S[1:, 1:] >= 0)).any())}
    return _seg_case(f"seg_u_spiral_{size}_size{speckle_size}_sub{int(subsampling)}", D, speckle_size, subsampling, facts)


def seg_serpent(W, H, speckle_size, subsampling):
    """Full rows joined alternately at their right and their left end: one segment whose union-find chain is H / 2 runs long."""
    D = np.full((H, W), INVALID, np.float32)
    D[0::2, :] = 5.0
    D[1::4, W - 1] = 5.0
    D[3::4, 0] = 5.0
    facts = _one_segment_facts(D, speckle_of(speckle_size, subsampling), W)
    facts["at least 130 rows"] = int(H >= 130)
    return _seg_case(f"seg_serpent_{W}x{H}_sub{int(subsampling)}", D, speckle_size, subsampling, facts)


def seg_skip_rule(W, speckle_size, subsampling, H=5):
    """The third condition of seg_link's skip rule: the pair to the left is similar and continues into the upper run, but
    the lower pixels are NOT one run, so this pair is the only link between the two runs.  The segment has exactly s pixels."""
    s = speckle_of(speckle_size, subsampling)
    L = s - 3
    D = np.full((H, W), INVALID, np.float32)
    facts = {"patterns placed": 0}
    for row, x in ((0, 0), (3, W - L - 1)):
        assert x + 1 + L <= W
        D[row, x], D[row, x + 1] = 5.0, 5.5
        D[row + 1, x] = 4.5
        D[row + 1, x + 1:x + 1 + L] = 6.0
        facts["patterns placed"] += 1
    hist = _size_histogram(D)
    facts[f"segments of exactly {s} pixels"] = int(hist[s]) if s < len(hist) else 0
    facts["nothing else"] = int(hist.sum() == 2)
    return _seg_case(f"seg_skip_rule_{W}x{H}_size{speckle_size}_sub{int(subsampling)}", D, speckle_size, subsampling, facts)


def seg_checkerboard(speckle_size, subsampling, H=8):
    """64 different disparities in every row of 64 pixels, no two neighbours similar: every lane of a wave has its own root."""
    u, v = np.meshgrid(np.arange(64), np.arange(H))
    D = (2.0 * ((u + 5 * v) % 64)).astype(np.float32)
    hist = _size_histogram(D)
    facts = {"every pixel a segment of its own": int(len(hist) == 2 and hist[1] == D.size),
             "64 different values per row": int(all(len(np.unique(r)) == 64 for r in D))}
    return _seg_case(f"seg_checkerboard_64x{H}_sub{int(subsampling)}", D, speckle_size, subsampling, facts)


def seg_random(W, H, speckle_size, subsampling, seed, first=0.5):
    """Two similarity classes ({0, 1}, a pixel's with probability `first`, and {2.5, 3.5}) and 15 % invalid pixels at random:
    segments of every size and shape."""
    rng = np.random.default_rng(seed)
    D = rng.choice(np.array([0.0, 1.0, 2.5, 3.5], np.float32), size=(H, W), p=[first / 2, first / 2, (1 - first) / 2, (1 - first) / 2])
    D[rng.random((H, W)) < 0.15] = INVALID
    facts = {"pixels": int(D.size)}
    if H >= 4:
        facts["invalid pixels"] = int((D < 0).sum())
        facts.update(_kept_removed(D, speckle_of(speckle_size, subsampling)))
    return _seg_case(f"seg_random_{W}x{H}_size{speckle_size}_sub{int(subsampling)}_seed{seed}", D, speckle_size, subsampling, facts)


def segment_cases():
    """Every removeSmallSegments case.  Widths around seg_rows' chunking (256 threads, ceil(W / 256) pixels each): 2, 63, 255,
    256, 257, 513; heights from 2 to the serpent's 131."""
    cases = []
    for (W, H, size, sub) in ((2, 60, 12, 0), (63, 30, 12, 1), (255, 24, 12, 0), (256, 30, 200, 1), (257, 60, 200, 0), (513, 60, 200, 0),
                              (513, 30, 200, 1), (513, 12, 12, 0)):
        cases.append(seg_sizes(W, H, size, sub, seed=W + size + sub))
    cases += [seg_threshold(63, 40, 12, 0), seg_threshold(257, 30, 200, 1), seg_threshold(513, 60, 200, 0), seg_threshold(255, 20, 12, 1)]
    cases += [seg_comb(63, 9, 200, 0, True), seg_comb(63, 9, 200, 0, False), seg_comb(97, 61, 200, 0, True), seg_comb(97, 61, 200, 0, False),
              seg_comb(21, 9, 200, 1, True), seg_comb(11, 9, 12, 0, False)]
    cases += [seg_two_runs(150, 200, 0, False), seg_two_runs(150, 200, 0, True), seg_two_runs(9, 12, 0, False), seg_two_runs(9, 12, 0, True),
              seg_two_runs(20, 200, 1, True), seg_two_runs(257, 200, 0, False, True), seg_two_runs(2, 12, 0, True, True)]
    cases += [seg_u_and_spiral(200, 0, 69), seg_u_and_spiral(200, 1, 25), seg_u_and_spiral(12, 0, 9)]
    cases += [seg_serpent(5, 131, 200, 0), seg_serpent(5, 131, 200, 1), seg_serpent(2, 131, 12, 0), seg_serpent(97, 133, 200, 0)]
    cases += [seg_skip_rule(63, 12, 0), seg_skip_rule(257, 200, 0), seg_skip_rule(63, 200, 1), seg_skip_rule(513, 200, 0), seg_skip_rule(257, 200, 0, 60), seg_skip_rule(256, 200, 1, 30)]
    cases += [seg_checkerboard(12, 0), seg_checkerboard(200, 1), seg_checkerboard(200, 0, 64), seg_checkerboard(200, 1, 64)]
    for (W, H, size, sub, seed) in ((2, 2, 12, 0, 1), (2, 131, 12, 1, 2), (63, 7, 12, 0, 3), (255, 5, 12, 1, 4), (256, 5, 12, 0, 5),
                                    (257, 5, 200, 1, 6), (513, 4, 12, 0, 7), (513, 2, 200, 1, 8), (97, 60, 200, 0, 9), (97, 60, 200, 1, 10)):
        cases.append(seg_random(W, H, size, sub, seed, first=0.8 if size == 200 else 0.5))
    return cases


# ------------------------------------------------------------------ gapInterpolation
def _runs(line_valid):
    """Maximal runs of invalid pixels of a line -> [(first, last)]."""
    runs, start = [], None
    for i, ok in enumerate(line_valid):
        if not ok and start is None:
            start = i
        if ok and start is not None:
            runs.append((start, i - 1))
            start = None
    if start is not None:
        runs.append((start, len(line_valid) - 1))
    return runs


def _gap_facts(D, g):
    facts = {}
    for axis, lines in (("rows", D), ("columns", D.T)):
        n = lines.shape[1]
        count = dict(g=0, g1=0, start=0, end=0, empty=0, single=0, three=0, three_down=0)
        for line in lines:
            valid = line >= 0
            count["empty"] += int(not valid.any())
            count["single"] += int(valid.sum() == 1)
            for first, last in _runs(valid):
                if first == 0 and last == n - 1:
                    continue
                count["start"] += int(first == 0)
                count["end"] += int(last == n - 1)
                if first > 0 and last < n - 1:
                    count["g"] += int(last - first + 1 == g)
                    count["g1"] += int(last - first + 1 == g + 1)
                    if last - first + 1 <= g:
                        diff = np.abs(line[first - 1] - line[last + 1])
                        count["three"] += int(diff == np.float32(3))
                        count["three_down"] += int(diff == THREE_DOWN)
        facts[f"{axis}: gaps of exactly {g} pixels between valid ones"] = count["g"]
        facts[f"{axis}: gaps of exactly {g + 1} pixels between valid ones"] = count["g1"]
        facts[f"{axis}: gaps that touch the line's start"] = count["start"]
        facts[f"{axis}: gaps that touch the line's end"] = count["end"]
        facts[f"{axis}: lines without a valid pixel"] = count["empty"]
        facts[f"{axis}: lines with a single valid pixel"] = count["single"]
        facts[f"{axis}: fillable gaps whose ends differ by exactly 3.0"] = count["three"]
        facts[f"{axis}: fillable gaps whose ends differ by nextafter(3.0, 0)"] = count["three_down"]
    return facts


def _gap_patterns(n, g, base):
    """Six lines of length n (rows of the result) that hold the gap patterns; base: valid values to carve from [6, n]."""
    P = base.copy()

    def carve(r, first, count):
        P[r, max(first, 0):max(min(first + count, n), 0)] = INVALID
    carve(0, 1, g)                       # a gap of g and one of g + 1 between valid pixels
    carve(0, g + 2, g + 1)
    k = min(g, max((n - 2) // 2, 1))     # gaps at both ends of the line
    carve(1, 0, k)
    carve(1, n - k, k)
    carve(2, 0, n)                       # no valid pixel
    carve(3, 0, n)                       # a single one
    P[3, n // 2] = 4.0
    if n >= 2 * g + 6:                   # a gap of g with ends 3.0 apart (the lower end is taken), one just below 3.0 (the mean)
        P[4, 0], P[4, 1 + g] = 4.0, 7.0
        carve(4, 1, g)
        a = g + 3
        P[4, a], P[4, a + 1 + g] = 0.0, THREE_DOWN
        carve(4, a + 1, g)
    carve(5, 2, 1)                       # a single pixel
    return P


def gap_lines(W, H, ipol_gap_width, subsampling, add_corners, seed, require=None):
    """Rows 0-5 (from column 7) and columns 0-5 (from row 7) hold the line patterns (gaps of g and g + 1, at the ends, empty and single-pixel lines, ends
    3.0 and just below 3.0 apart); the rest: random holes and plus-shaped holes, where the row pass fills what the column pass
    then sees."""
    g = gap_of(ipol_gap_width, subsampling)
    rng = np.random.default_rng(seed)
    D = (rng.integers(0, 12, (H, W)) + rng.choice([0.0, 0.25, 0.5], size=(H, W))).astype(np.float32)
    D[7:, 7:][rng.random((H - 7, W - 7)) < 0.12] = INVALID
    plus = 0
    for y in range(10, H - 3, 7):
        for x in range(10, W - 3, 9):
            D[y - 2:y + 3, x - 2:x + 3] = 6.0
            D[y, x - 1:x + 2] = INVALID
            D[y - 1:y + 2, x] = INVALID
            plus += 1
    D[6, :], D[:, 6] = 2.0, 2.0                      # (valid lines between the pattern lines and the rest)
    D[:7, :7] = INVALID                              # (the corner: every pattern line starts with seven invalid pixels)
    D[:6, 7:] = _gap_patterns(W - 7, g, D[:6, 7:])
    D[7:, :6] = _gap_patterns(H - 7, g, np.ascontiguousarray(D[7:, :6].T)).T
    facts = _gap_facts(D, g)
    facts["plus-shaped holes"] = plus
    if require is not None:
        facts = {k: v for k, v in facts.items() if any(r in k for r in require)}
    w, h = image_size(D.shape, subsampling)
    return dict(name=f"gap_{W}x{H}_width{ipol_gap_width}_sub{int(subsampling)}_corners{int(add_corners)}", stage="gap", D=D,
                ipol_gap_width=ipol_gap_width, add_corners=bool(add_corners), subsampling=bool(subsampling), width=w, height=h, facts=facts)


def gap_cases():
    """ROBOTICS (3 pixels; 2 with subsampling), MIDDLEBURY (5000, add_corners: every line is shorter than the gap), and 64 / 65
    without add_corners: the widest gap of the pixel-per-thread kernels and the narrowest of the line walk."""
    short = ("line's start", "line's end", "without a valid", "single valid", "plus")   # what a line shorter than the gap can hold
    tiny = ("line's start", "without a valid")
    cases = [gap_lines(97, 60, 3, 0, 0, 1), gap_lines(63, 33, 3, 1, 0, 2), gap_lines(257, 60, 3, 0, 0, 3), gap_lines(256, 30, 3, 1, 0, 4),
             gap_lines(97, 60, 5000, 0, 1, 5, short), gap_lines(97, 33, 5000, 1, 1, 6, short), gap_lines(63, 33, 3, 0, 1, 7),
             gap_lines(144, 144, 64, 0, 0, 8), gap_lines(144, 144, 65, 0, 0, 9), gap_lines(40, 30, 64, 0, 0, 10, short),
             gap_lines(40, 30, 65, 0, 0, 11, short), gap_lines(9, 9, 3, 0, 0, 12, tiny), gap_lines(8, 8, 5000, 0, 1, 13, tiny)]
    return cases


# ------------------------------------------------------------------ adaptiveMean
def mean_map(W, H, subsampling, seed):
    """The mixture of test_adaptive_mean_alone_on_synthetic_maps_equals_the_reference_source: a ramp, steps of 2 / 4 / 8 / 16
    levels (the exponent classes of the subsampling branch's mask), invalid pixels at -1, an island at -10."""
    rng = np.random.default_rng(seed)
    D = (np.linspace(0, 60, W)[None, :] + np.linspace(0, 9, H)[:, None]).astype(np.float32)
    D += rng.choice([0, 0, 0, 2, 4, 8, 16, 33.5], size=D.shape).astype(np.float32)
    D[rng.random(D.shape) < 0.15] = -1.0
    if H >= 9 and W >= 8:
        D[H // 3:H // 3 + 3, W // 4:W // 2] = INVALID
    w, h = image_size(D.shape, subsampling, odd=True)
    taps = 4 if subsampling else 8
    # the vertical pass, the only one that writes D, covers columns 3 .. W - 4 and needs `taps` rows: `untouched` = it writes nothing
    return dict(name=f"mean_{W}x{H}_sub{int(subsampling)}", stage="mean", D=D, subsampling=bool(subsampling), width=w, height=h,
                untouched=W < 7 or H < taps, facts={"valid pixels": int((D >= 0).sum())})


def mean_cases():
    """H and W in {2, 6, 7, 8, 9} (the 8-tap window needs 8 pixels, the passes skip three lines at either border) and one
    larger map; both tap counts (8: full resolution, 4: subsampling)."""
    cases = []
    for sub in (0, 1):
        for H in (2, 6, 7, 8, 9):
            for W in (2, 6, 7, 8, 9):
                cases.append(mean_map(W, H, sub, seed=100 * H + W + sub))
        cases.append(mean_map(131, 77, sub, seed=5 + sub))
    return cases


# ------------------------------------------------------------------ leftRightConsistencyCheck
def lr_maps(W, H, subsampling, lr_threshold, seed):
    """Rows 0-4: disparities that warp to exactly column 0, to W - 1, (with subsampling) to -0.5 and W - 0.5, and beyond the
    image; the rest: pairs that agree, that differ by exactly the threshold, by one more and by the next float."""
    assert H >= 8
    rng = np.random.default_rng(seed)
    half = np.float32(2.0 if subsampling else 1.0)       # disparity per column of the map
    u = np.arange(W, dtype=np.float32)
    D1 = np.full((H, W), INVALID, np.float32)
    D2 = np.full((H, W), INVALID, np.float32)
    D1[0] = u * half                                     # u - d1 (/ 2) = 0
    D2[0] = rng.choice([0.0, 1.0, 2.0, 40.0], size=W)
    D2[1] = (W - 1 - u) * half                           # u + d2 (/ 2) = W - 1
    D1[1] = rng.choice([0.0, 1.0, 2.0, 40.0], size=W)
    D1[2] = 2 * u + 1                                    # subsampling: -0.5 (outside); full resolution: further outside
    D2[2] = 1.0
    D2[3] = 2 * (W - u) - 1                              # subsampling: W - 0.5 (inside, truncated to W - 1)
    D1[3] = D2[3, ::-1]
    D1[4] = (W + 5 + u) * half                           # larger than the image is wide
    D2[4] = (W + 5 + u) * half
    deltas = np.array([0, 0, lr_threshold, -lr_threshold, lr_threshold + 1, -(lr_threshold + 1),
                       np.nextafter(np.float32(lr_threshold), np.float32(99))], np.float32)
    for v in range(5, H):
        d1 = (rng.integers(0, 12, W) + rng.choice([0.0, 0.0, 0.5, 0.75], size=W)).astype(np.float32)      # (fractions: where
        D1[v] = d1                                                                                         # truncating is not rounding)
        D2[v] = (rng.integers(0, 12, W) + rng.choice([0.0, 0.0, 0.5, 0.75], size=W)).astype(np.float32)
        for x in rng.permutation(W):                     # the pixel of the other map that x's disparity points to: set to d1 + delta
            t = x - d1[x] / half
            if 0 <= t < W:
                D2[v, int(t)] = max(d1[x] + rng.choice(deltas), np.float32(0))
        D1[v][rng.random(W) < 0.1] = INVALID
        D2[v][rng.random(W) < 0.1] = -1.0
    warp1, warp2 = u[None, :] - D1 / half, u[None, :] + D2 / half
    ok1 = (D1 >= 0) & (warp1 >= 0) & (warp1 < W)
    diff1 = np.abs(np.take_along_axis(D2, np.clip(warp1, 0, W - 1).astype(np.int64), axis=1) - D1)
    facts = {"left pixels that warp to exactly column 0": int(((D1 >= 0) & (warp1 == 0)).sum()),
             "right pixels that warp to exactly column W - 1": int(((D2 >= 0) & (warp2 == W - 1)).sum()),
             "disparities larger than the map is wide": int((D1 > W * half).sum()),
             "pairs that differ by exactly lr_threshold": int((ok1 & (diff1 == lr_threshold)).sum()),
             "pairs that differ by lr_threshold + 1": int((ok1 & (diff1 == lr_threshold + 1)).sum()),
             "pairs that differ by the float after lr_threshold": int((ok1 & (diff1 == deltas[-1])).sum())}
    frac1, frac2 = warp1 - np.floor(warp1), warp2 - np.floor(warp2)
    facts["warped columns whose fraction is 0.5 or more (truncated, not rounded)"] = int(
        (ok1 & (frac1 >= 0.5)).sum() + ((D2 >= 0) & (warp2 < W) & (frac2 >= 0.5)).sum())
    if W < 32:       # (too few pixels for every delta to land)
        facts = {k: v for k, v in facts.items() if "differ" not in k}
    if subsampling:
        facts["left pixels that warp to -0.5"] = int(((D1 >= 0) & (warp1 == -0.5)).sum())
        facts["right pixels that warp to W - 0.5"] = int(((D2 >= 0) & (warp2 == W - 0.5)).sum())
    w, h = image_size(D1.shape, subsampling)
    return dict(name=f"lr_{W}x{H}_sub{int(subsampling)}_thr{lr_threshold}", stage="lr", D1=D1, D2=D2, subsampling=bool(subsampling),
                lr_threshold=lr_threshold, width=w, height=h, facts=facts)


def lr_cases():
    return [lr_maps(97, 60, 0, 2, 1), lr_maps(63, 30, 1, 2, 2), lr_maps(257, 60, 0, 2, 3), lr_maps(256, 30, 1, 2, 4),
            lr_maps(9, 8, 0, 2, 5), lr_maps(9, 8, 1, 2, 6), lr_maps(63, 20, 0, 1, 7), lr_maps(63, 20, 1, 5, 8)]


# ------------------------------------------------------------------ a chain of stages on one mixed map pair
def chain_case(subsampling, seed=11):
    """A pair for the chain lr -> seg -> gap -> mean: smooth maps that mostly agree, holes, speckles, -1 and -10."""
    W, H = 131, 77
    rng = np.random.default_rng(seed)
    half = 2.0 if subsampling else 1.0
    base = np.round(6 + 4 * np.sin(np.arange(W) / 17.0)[None, :] + np.arange(H)[:, None] / 20.0).astype(np.float32)
    D1, D2 = base.copy(), base.copy()
    for v in range(H):
        for x in range(W):
            t = int(x - base[v, x] / half)
            if 0 <= t < W:
                D2[v, t] = base[v, x]
    D1 += rng.choice([0, 0, 0, 0, 1, 3, 7], size=D1.shape).astype(np.float32)
    D1[rng.random(D1.shape) < 0.1] = -1.0
    D2[rng.random(D2.shape) < 0.1] = -1.0
    D1[20:24, 30:60] = INVALID
    w, h = image_size(D1.shape, subsampling)
    return dict(name=f"chain_sub{int(subsampling)}", stage="chain", D1=D1, D2=D2, subsampling=bool(subsampling), width=w, height=h,
                facts={"valid pixels": int((D1 >= 0).sum())})


# ------------------------------------------------------------------ computeDisparity's triangle loop
def _plane(points):
    """d = a * x + b * y + c through three (x, y, d); a singular system: the constant plane through their mean."""
    A = np.array([[x, y, 1.0] for x, y, _ in points], np.float64)
    d = np.array([p[2] for p in points], np.float64)
    if abs(np.linalg.det(A)) < 1e-9:
        return 0.0, 0.0, float(d.mean())
    return tuple(np.linalg.solve(A, d))


def make_triangles(support, corners):
    """TRIANGLE records over `support` for the corner triples, with the planes of the left (u) and the right (u - d) image."""
    from tests.elas_ref import TRIANGLE
    tri = np.zeros(len(corners), TRIANGLE)
    for i, c in enumerate(corners):
        p = [support[k] for k in c]
        tri[i]["c1"], tri[i]["c2"], tri[i]["c3"] = c
        tri[i]["t1a"], tri[i]["t1b"], tri[i]["t1c"] = _plane([(q["u"], q["v"], q["d"]) for q in p])
        tri[i]["t2a"], tri[i]["t2b"], tri[i]["t2c"] = _plane([(q["u"] - q["d"], q["v"], q["d"]) for q in p])
    return tri


def triangle_cases(calls, seed=7):
    """Triangle lists on the committed capture's two calls (left and right image).  -> [case]: each holds `calls`, the two
    argument dicts with `support` / `tri` replaced.  Every corner keeps 0 <= v < height."""
    from tests.elas_ref import SUPPORT
    rng = np.random.default_rng(seed)
    width, height = calls[0]["width"], calls[0]["height"]
    n = len(calls[0]["support"])
    assert all(np.array_equal(c["support"], calls[0]["support"]) for c in calls)
    extra_pts = np.array([(50, 10, 20), (50, 90, 22), (120, 60, 25),        # two corners in one column
                          (30, 30, 10), (60, 60, 12), (90, 90, 14),         # three in one line
                          (0, 5, 0), (width - 1, 64, 3), (100, 0, 8), (140, height - 1, 9),   # one on each border
                          (10, 40, 60), (25, 100, 90), (40, 70, 45)],       # u - d < 0 in the right image
                         dtype=SUPPORT)
    support = np.concatenate([calls[0]["support"], extra_pts])
    assert (support["v"] >= 0).all() and (support["v"] < height).all()
    over = [tuple(int(k) for k in rng.choice(n, 3, replace=False)) for _ in range(40)]
    degenerate = [(n, n + 1, n + 2), (n + 3, n + 4, n + 5), (n + 3, n + 3, n + 3), (n, n, n + 2), (n + 6, n + 7, n + 8), (n + 6, n + 9, n + 7),
                  (n + 8, n + 9, n + 6), (n + 10, n + 11, n + 12), (n + 10, n + 2, n + 11)]
    steep = make_triangles(support, over[:6])
    steep["t1a"], steep["t2a"] = [0.9, -0.7, 0.7, 0.1, -0.2, 3.0], [0.1, 0.2, -0.9, 0.7, -0.7, 0.0]
    extra = np.concatenate([make_triangles(support, over), make_triangles(support, degenerate), steep])
    cases = []

    def case(name, lists, **facts):
        cases.append(dict(name=name, stage="tri", calls=[dict({k: v for k, v in c.items() if k != "D"}, support=support, tri=np.ascontiguousarray(t))
                                                    for c, t in zip(calls, lists)],
                          facts=facts))
    perm = [rng.permutation(len(c["tri"])) for c in calls]
    case("tri_capture", [c["tri"] for c in calls], triangles=len(calls[0]["tri"]))
    case("tri_capture_shuffled", [c["tri"][p] for c, p in zip(calls, perm)], moved=int(sum((p != np.arange(len(p))).sum() for p in perm)))
    case("tri_appended", [np.concatenate([c["tri"], extra]) for c in calls], appended=len(extra),
         steep_planes=int((np.abs(extra["t1a"]) >= 0.7).sum()), right_corners_left_of_the_image=int((support["u"] - support["d"] < 0).sum()))
    case("tri_appended_reversed", [np.concatenate([c["tri"], extra[::-1]]) for c in calls], appended=len(extra))
    case("tri_prepended", [np.concatenate([extra, c["tri"]]) for c in calls], appended=len(extra))
    both = [np.concatenate([c["tri"], extra]) for c in calls]
    case("tri_all_shuffled", [b[rng.permutation(len(b))] for b in both], triangles=len(both[0]))
    case("tri_degenerate_only", [make_triangles(support, degenerate) for _ in calls], triangles=len(degenerate))
    return cases


TRI_SETTINGS = [dict(subsampling=0, match_texture=1), dict(subsampling=1, match_texture=1), dict(subsampling=0, match_texture=0),
                dict(subsampling=0, match_texture=10000), dict(subsampling=1, match_texture=0)]


def map_cases():
    return segment_cases() + gap_cases() + mean_cases() + lr_cases()
