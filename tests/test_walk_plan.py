"""The policy of the order-free chisel integrate (plvs_amd/csrc/tsdf_walk_plan.hpp) on a CPU: plan_walk_call, sort_kind and
adapt_after_call against plans written out by hand and against a restatement of the rules over a grid of calls.

T = tiles, a = attempt, M = collect mode (0 never / 1 long calls / 2 every call), E = the runs of the call before scaled to
this call's tiles.  Lists a, b, c of deferred tiles are 0, 1, 2; -1 = a pass over every tile.
"""
import itertools
import os
import shutil

import numpy as np
import pytest

from tests import oracle_lib

SMALL, MEDIUM, GENERAL = 0, 1, 2
OWN, PREDICTED, COLLECTED = 0, 1, 2
FIELDS = ("size_class npasses e0 g0 s0 d0 e1 g1 s1 d1 e2 g2 s2 d2 last_list pieces chain collect_ready collect_any_count "
          "serial_small apply_on_side record_fork scan_first run_bound chunk_bound collect_rows "
          "collect_blocks collect_bound parts_cap").split()


def call(T, a=0, max_chunks=20000, chunks_before=1000, r1=11, known=True, runs_last=0, tiles_last=None, last_updated=100,
         walk_small=False, third_pass=False, M=1, max_rows=0):
    """The inputs of one attempt; tiles_last defaults to T, so that E = runs_last."""
    return dict(T=T, a=a, max_chunks=max_chunks, chunks_before=chunks_before, r1=r1, known=known, runs_last=runs_last,
                tiles_last=T if tiles_last is None else tiles_last, last_updated=last_updated, walk_small=walk_small,
                third_pass=third_pass, M=M, max_rows=max_rows)


def pack(c):
    return np.array([c["T"], c["a"], c["max_chunks"], c["chunks_before"], c["r1"], c["known"], c["runs_last"], c["tiles_last"],
                     c["last_updated"], c["walk_small"], c["third_pass"], c["M"], c["max_rows"]], np.int64)


@pytest.fixture(scope="module", params=["g++", "rocm-clang"])
def lib(request):
    if request.param == "rocm-clang":
        if not os.path.exists(oracle_lib.ROCM_CLANG):
            pytest.skip("no ROCm clang on this machine")
        old = os.environ.get("PLVS_HOST_CXX")
        os.environ["PLVS_HOST_CXX"] = "rocm-clang"
        try:
            yield oracle_lib.load_hostplan()
        finally:
            if old is None:
                del os.environ["PLVS_HOST_CXX"]
            else:
                os.environ["PLVS_HOST_CXX"] = old
    else:
        if shutil.which("g++") is None:
            pytest.skip("no g++ on this machine")
        yield oracle_lib.load_hostplan()


def plan(lib, c):
    out = np.full(len(FIELDS), -12345, np.int64)
    lib.hostplan_plan(oracle_lib._ptr(pack(c)), oracle_lib._ptr(out))
    return dict(zip(FIELDS, (int(v) for v in out)))


def sort_kind(D, T):
    return SMALL if D <= 4096 else MEDIUM if (T <= 2048 and D <= 16384) else GENERAL


def restated(c):
    """The rules, restated: every field of the plan of one attempt."""
    T, a, M, known = c["T"], c["a"], c["M"], bool(c["known"])
    scaled = float(c["runs_last"]) * float(T) / float(max(1, c["tiles_last"]))
    E = int(scaled) if known else None
    p = dict.fromkeys(FIELDS, 0)
    p["size_class"] = 0 if T <= 320 else 1 if T <= 4096 else 2
    if T <= 320:
        passes = [(4096, T, -1, 0)]
    elif c["walk_small"]:
        passes = [(1024, T, -1, 0), (2048, min(T, 1024), 0, 1)] + ([(4096, min(T, 512), 1, 2)] if c["third_pass"] else [])
    else:
        passes = [(2048, T, -1, 0), (4096, min(T, 512), 0, 1)]
    p["npasses"] = len(passes)
    for i, (e, g, s, d) in enumerate(passes):
        p[f"e{i}"], p[f"g{i}"], p[f"s{i}"], p[f"d{i}"] = e, g, s, d
    p["last_list"] = passes[-1][3]
    p["pieces"] = 1 if (T > 320 and c["walk_small"] and not c["third_pass"]) else 2
    predicted = known and a == 0 and M != 2 and (T <= 4096 or (E <= 200000 and M == 0))
    collect_ready = M != 0 and (T > 4096 or M == 2) and not predicted
    collect_fast = collect_ready and known and a == 0
    p["chain"] = PREDICTED if predicted else COLLECTED if collect_fast else OWN
    p["collect_ready"] = int(collect_ready)
    p["collect_any_count"] = int(M == 2)
    serial_small = predicted and E <= 2048
    p["serial_small"] = int(serial_small)
    p["apply_on_side"] = int(predicted and not serial_small)
    p["record_fork"] = int(not collect_fast)
    if predicted:
        run_bound = 4096 if E <= 2048 else min(T << c["r1"], (E * 5 // 4 + 8191) // 4096 * 4096)
        if T <= 2048 and run_bound > 4096 and E * 5 // 4 + 1024 <= 16384:
            run_bound = 16384
        p["run_bound"] = run_bound
        p["chunk_bound"] = min(c["max_chunks"], max(2 * c["chunks_before"], c["chunks_before"] + 256))
        p["scan_first"] = int(sort_kind(run_bound, T) == GENERAL)
    row_chunks = 256
    while row_chunks < 2 * c["last_updated"] + 64:
        row_chunks *= 2
    if c["max_rows"] > 0:
        row_chunks = min(row_chunks, c["max_rows"])
    p["collect_rows"] = min(c["max_chunks"], row_chunks) * 8
    p["collect_blocks"] = -(-T * 64 // 1024)
    p["collect_bound"] = min(T << c["r1"], max(8 << 20, int(4.0 * float(c["runs_last"]) * float(T) / float(max(1, c["tiles_last"]))) if known else 0))
    p["parts_cap"] = p["collect_bound"] // 4096 + p["collect_rows"] + 1
    return p


# (case, the fields written out)
LEAN_SMALL = dict(size_class=0, npasses=1, e0=4096, s0=-1, d0=0, last_list=0, pieces=2)
LEAN_2048 = dict(npasses=2, e0=2048, s0=-1, d0=0, e1=4096, s1=0, d1=1, last_list=1, pieces=2)
LEAN_1024 = dict(npasses=2, e0=1024, s0=-1, d0=0, e1=2048, s1=0, d1=1, last_list=1, pieces=1)
LEAN_THREE = dict(npasses=3, e0=1024, s0=-1, d0=0, e1=2048, s1=0, d1=1, e2=4096, s2=1, d2=2, last_list=2, pieces=2)
FIRST_CALL = dict(chain=OWN, serial_small=0, apply_on_side=0, record_fork=1, scan_first=0,
                  run_bound=0, chunk_bound=0)
SERIAL = dict(chain=PREDICTED, collect_ready=0, serial_small=1, apply_on_side=0, record_fork=1, scan_first=0,
              run_bound=4096, chunk_bound=2000)
FORKED = dict(chain=PREDICTED, collect_ready=0, serial_small=0, apply_on_side=1, record_fork=1, chunk_bound=2000)
QUEUED = dict(chain=COLLECTED, collect_ready=1, serial_small=0, apply_on_side=0, record_fork=0, scan_first=0,
              run_bound=0)
OWN_COUNTS = dict(chain=OWN, serial_small=0, apply_on_side=0, record_fork=1, scan_first=0, run_bound=0)
CASES = [
    # a handle's first call: small, mid, long
    (call(150, known=False), dict(LEAN_SMALL, g0=150, collect_ready=0, **FIRST_CALL)),
    (call(3000, known=False), dict(LEAN_2048, size_class=1, g0=3000, g1=512, collect_ready=0, **FIRST_CALL)),
    (call(15000, known=False), dict(LEAN_2048, size_class=2, g0=15000, g1=512, collect_ready=1, collect_bound=8 << 20,
                                    collect_blocks=938, collect_rows=512 * 8, parts_cap=2048 + 4096 + 1, **FIRST_CALL)),
    (call(15000, known=False, M=0), dict(collect_ready=0, **FIRST_CALL)),
    (call(150, known=False, M=2), dict(collect_ready=1, collect_any_count=1, **FIRST_CALL)),
    # known history, the size classes and the lean passes on both sides of 320
    (call(150, runs_last=500), dict(LEAN_SMALL, g0=150, **SERIAL)),
    (call(320, runs_last=500, walk_small=True, third_pass=True), dict(LEAN_SMALL, g0=320, **SERIAL)),
    (call(321, runs_last=500), dict(LEAN_2048, size_class=1, g0=321, g1=321, **SERIAL)),
    (call(321, runs_last=500, walk_small=True), dict(LEAN_1024, size_class=1, g0=321, g1=321, **SERIAL)),
    (call(2048, runs_last=500, walk_small=True), dict(LEAN_1024, size_class=1, g0=2048, g1=1024, **SERIAL)),
    (call(2049, runs_last=500, walk_small=True, third_pass=True), dict(LEAN_THREE, size_class=1, g0=2049, g1=1024, g2=512, **SERIAL)),
    (call(4096, runs_last=500, third_pass=True), dict(LEAN_2048, size_class=1, g0=4096, g1=512, **SERIAL)),
    # E on both sides of 2048: everything on the caller's stream / the apply stage on the side stream
    (call(150, runs_last=2048), dict(SERIAL)),
    (call(150, runs_last=2049), dict(FORKED, run_bound=16384, scan_first=0)),    # (one-workgroup sort)
    (call(2048, runs_last=2049), dict(FORKED, run_bound=16384, scan_first=0)),
    (call(2049, runs_last=2048), dict(SERIAL)),
    # 2048 < T <= 4096 with 4096 < run_bound <= 16384: the general chain, whose compaction reads the scanned counts
    (call(2049, runs_last=2049), dict(FORKED, run_bound=8192, scan_first=1)),
    (call(3000, runs_last=6000), dict(FORKED, run_bound=12288, scan_first=1)),
    (call(4096, runs_last=9830), dict(FORKED, run_bound=16384, scan_first=1)),
    (call(4096, runs_last=9832), dict(FORKED, run_bound=20480, scan_first=1)),
    # ... and of few tiles: the one-workgroup sort up to E * 5 / 4 + 1024 <= 16384, the general chain beyond
    (call(2048, runs_last=9830), dict(FORKED, run_bound=16384, scan_first=0)),
    (call(2048, runs_last=12288), dict(FORKED, run_bound=16384, scan_first=0)),
    (call(2048, runs_last=12289), dict(FORKED, run_bound=20480, scan_first=1)),
    (call(2048, runs_last=13107), dict(FORKED, run_bound=20480, scan_first=1)),     # 16384 * 4 / 5
    (call(2048, runs_last=13108), dict(FORKED, run_bound=24576, scan_first=1)),
    (call(4, runs_last=9000), dict(FORKED, run_bound=16384, scan_first=0)),
    (call(4, runs_last=13000), dict(FORKED, run_bound=8192, scan_first=0)),          # (the tiles' run slots bound it)
    # E scaled from a call of another length
    (call(3000, runs_last=100, tiles_last=150), dict(SERIAL)),
    (call(150, runs_last=1_000_000, tiles_last=15000), dict(FORKED, run_bound=16384, scan_first=0)),
    # long calls: collected and queued (M = 1), predicted up to 200 000 runs (M = 0), never predicted (M = 2)
    (call(4097, runs_last=500), dict(LEAN_2048, size_class=2, g0=4097, g1=512, collect_bound=8 << 20, **QUEUED)),
    (call(15000, runs_last=3_000_000), dict(QUEUED, size_class=2, collect_bound=12_000_000, collect_blocks=938,
                                            parts_cap=12_000_000 // 4096 + 4096 + 1)),
    (call(15000, runs_last=200000, M=0), dict(FORKED, size_class=2, run_bound=258048, scan_first=1)),
    (call(15000, runs_last=200001, M=0), dict(OWN_COUNTS, collect_ready=0)),
    (call(15000, runs_last=500, M=0), dict(SERIAL, size_class=2)),
    (call(15000, runs_last=500, M=2), dict(QUEUED, collect_any_count=1)),
    (call(150, runs_last=500, M=2), dict(LEAN_SMALL, g0=150, **dict(QUEUED, collect_any_count=1))),
    (call(3000, runs_last=500, M=0), dict(SERIAL)),
    # attempt 1: never predicted, never queued without a read
    (call(150, a=1, runs_last=500), dict(OWN_COUNTS, collect_ready=0)),
    (call(3000, a=1, runs_last=6000), dict(OWN_COUNTS, collect_ready=0)),
    (call(15000, a=1, runs_last=500), dict(OWN_COUNTS, collect_ready=1)),
    (call(15000, a=1, runs_last=500, M=0), dict(OWN_COUNTS, collect_ready=0)),
    (call(150, a=1, runs_last=500, M=2), dict(OWN_COUNTS, collect_ready=1, collect_any_count=1)),
    # the run matrix: twice the chunks of the call before as a power of two, MAX_ROWS, max_chunks
    (call(15000, runs_last=500, last_updated=0), dict(collect_rows=256 * 8)),
    (call(15000, runs_last=500, last_updated=96), dict(collect_rows=256 * 8)),
    (call(15000, runs_last=500, last_updated=97), dict(collect_rows=512 * 8)),
    (call(15000, runs_last=500, last_updated=1000), dict(collect_rows=4096 * 8, parts_cap=2048 + 4096 * 8 + 1)),
    (call(15000, runs_last=500, last_updated=1000, max_rows=8), dict(collect_rows=64, parts_cap=2048 + 64 + 1)),
    (call(15000, runs_last=500, last_updated=1000, max_chunks=100), dict(collect_rows=800, chunk_bound=0)),
    (call(15000, runs_last=500, last_updated=1000, max_chunks=100, max_rows=8), dict(collect_rows=64)),
    # bounds: the chunks a predicted chain allows for, the run slots of the tiles
    (call(150, runs_last=500, chunks_before=100), dict(chunk_bound=356)),
    (call(150, runs_last=500, chunks_before=19990), dict(chunk_bound=20000)),
    (call(600, runs_last=2_000_000), dict(FORKED, run_bound=600 << 11, scan_first=1)),
    (call(600, runs_last=2_000_000, r1=12), dict(FORKED, run_bound=600 << 12, scan_first=1)),
    (call(600, runs_last=2_000_000, r1=13), dict(FORKED, run_bound=(2_500_000 + 8191) // 4096 * 4096, scan_first=1)),
    (call(1000, runs_last=9_000_000, M=2), dict(collect_bound=1000 << 11)),
]


def test_plans_written_out(lib):
    for c, want in CASES:
        got = plan(lib, c)
        for k, v in want.items():
            assert got[k] == v, (c, k, got[k], v)
        assert got == restated(c), c
        # the scan is queued in front of a predicted chain exactly when its sort is the general one
        if got["chain"] == PREDICTED:
            assert bool(got["scan_first"]) == (lib.hostplan_sort_kind(got["run_bound"], c["T"]) == GENERAL), c
            assert bool(got["scan_first"]) == bool(lib.hostplan_sort_needs_scan(got["run_bound"], c["T"])), c
        else:
            assert got["scan_first"] == 0 and got["run_bound"] == 0, c


def test_plans_over_a_grid_of_calls(lib):
    n = 0
    for T, runs, M, a, known, ws, tp in itertools.product(
            (1, 150, 320, 321, 600, 2048, 2049, 4096, 4097, 15000), (0, 2048, 2049, 9830, 9832, 12288, 12289, 13107, 13108, 65536,
                                                                      200000, 200001, 5_000_000),
            (0, 1, 2), (0, 1), (False, True), (False, True), (False, True)):
        for tiles_last, max_rows, last_updated in ((T, 0, 100), (150, 8, 3000), (15000, 0, 0)):
            c = call(T, a=a, known=known, runs_last=runs, tiles_last=tiles_last, walk_small=ws, third_pass=tp, M=M, max_rows=max_rows,
                     last_updated=last_updated)
            got = plan(lib, c)
            assert got == restated(c), c
            assert bool(got["scan_first"]) == (got["chain"] == PREDICTED and lib.hostplan_sort_kind(got["run_bound"], T) == GENERAL), c
            assert (got["chain"] == COLLECTED) <= bool(got["collect_ready"]), c
            assert a == 0 or got["chain"] == OWN, c
            n += 1
    assert n > 9000


def test_sort_kind(lib):
    table = [(0, 150, SMALL), (4096, 15000, SMALL), (4097, 150, MEDIUM), (4097, 2048, MEDIUM), (4097, 2049, GENERAL),
             (16384, 2048, MEDIUM), (16384, 2049, GENERAL), (16384, 4096, GENERAL), (16385, 150, GENERAL), (16385, 2048, GENERAL),
             (3_000_000, 15000, GENERAL)]
    for D, T, kind in table:
        assert lib.hostplan_sort_kind(D, T) == kind, (D, T)
        assert lib.hostplan_sort_needs_scan(D, T) == int(kind == GENERAL), (D, T)
    for D, T in itertools.product((0, 1, 4095, 4096, 4097, 8192, 16383, 16384, 16385, 65536, 1 << 22), (1, 320, 2047, 2048, 2049, 4096, 15000)):
        assert lib.hostplan_sort_kind(D, T) == sort_kind(D, T)
        assert lib.hostplan_sort_needs_scan(D, T) == int(sort_kind(D, T) == GENERAL)


def test_collected_on_the_calls_own_counts(lib):
    own = oracle_lib._ptr(pack(call(15000, known=False)))               # a long first call: the buffers are reserved
    assert lib.hostplan_collect_on_own_counts(own, 0, 0, 65537) == 1
    assert lib.hostplan_collect_on_own_counts(own, 0, 0, 65536) == 0   # too few runs to pay the chain's launches
    assert lib.hostplan_collect_on_own_counts(own, 1, 0, 65537) == 0   # a tile went to walk_tiles
    assert lib.hostplan_collect_on_own_counts(own, 0, 1, 65537) == 0   # a segment spilled
    every = oracle_lib._ptr(pack(call(150, known=False, M=2)))
    assert lib.hostplan_collect_on_own_counts(every, 0, 0, 1) == 1
    assert lib.hostplan_collect_on_own_counts(every, 0, 0, 0) == 1
    assert lib.hostplan_collect_on_own_counts(every, 2, 0, 1) == 0
    never = oracle_lib._ptr(pack(call(15000, known=False, M=0)))
    assert lib.hostplan_collect_on_own_counts(never, 0, 0, 1 << 20) == 0
    mid = oracle_lib._ptr(pack(call(3000, known=False)))
    assert lib.hostplan_collect_on_own_counts(mid, 0, 0, 1 << 20) == 0


def adapt(lib, hist, outcome, T):
    h = np.array(hist, np.int64)
    lib.hostplan_adapt(oracle_lib._ptr(h), oracle_lib._ptr(np.array(outcome, np.int64)), T)
    return [int(v) for v in h]


def test_feedback_after_a_call(lib):
    # hist: known, runs_last, tiles_last, walk_small, third_pass; outcome: runs, ndeferred, ndeferred2, over_small
    # the 2048-entry first pass counts the tiles a 1024-entry table would not have held: at most a sixth -> the small table
    assert adapt(lib, [0, 0, 1, 0, 0], [777, 5, 0, 500], 3000) == [1, 777, 3000, 1, 0]
    assert adapt(lib, [0, 0, 1, 0, 0], [777, 5, 0, 501], 3000) == [1, 777, 3000, 0, 0]
    assert adapt(lib, [1, 9, 9, 0, 1], [0, 0, 7, 0], 321) == [1, 0, 321, 1, 1]          # (third_pass: untouched by such a call)
    # the 1024-entry first pass: more than a quarter of the tiles deferred -> back to 2048; third_pass = the second pass deferred
    assert adapt(lib, [1, 9, 9, 1, 0], [50, 750, 0, 0], 3000) == [1, 50, 3000, 1, 0]
    assert adapt(lib, [1, 9, 9, 1, 0], [50, 751, 0, 0], 3000) == [1, 50, 3000, 0, 0]
    assert adapt(lib, [1, 9, 9, 1, 0], [50, 10, 3, 0], 3000) == [1, 50, 3000, 1, 1]
    assert adapt(lib, [1, 9, 9, 1, 1], [50, 10, 0, 0], 3000) == [1, 50, 3000, 1, 0]
    assert adapt(lib, [1, 9, 9, 1, 1], [50, 751, 3, 0], 15000 // 5) == [1, 50, 3000, 0, 1]
    # a small call walks with the 4096-entry table: it leaves the tables of the longer calls alone
    assert adapt(lib, [1, 9, 9, 1, 1], [50, 300, 0, 0], 320) == [1, 50, 320, 1, 1]
    assert adapt(lib, [0, 0, 1, 0, 0], [50, 0, 0, 0], 320) == [1, 50, 320, 0, 0]
    # and the plans follow
    c = call(3000, runs_last=500)
    assert plan(lib, c)["e0"] == 2048
    h = adapt(lib, [1, 500, 3000, 0, 0], [500, 0, 0, 10], 3000)
    nxt = plan(lib, call(3000, runs_last=h[1], tiles_last=h[2], walk_small=h[3], third_pass=h[4]))
    assert (nxt["e0"], nxt["e1"], nxt["npasses"], nxt["pieces"]) == (1024, 2048, 2, 1)
    h = adapt(lib, h, [500, 40, 2, 0], 3000)
    nxt = plan(lib, call(3000, runs_last=h[1], tiles_last=h[2], walk_small=h[3], third_pass=h[4]))
    assert (nxt["npasses"], nxt["e2"], nxt["last_list"], nxt["pieces"]) == (3, 4096, 2, 2)
