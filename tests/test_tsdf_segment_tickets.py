"""Segment tickets (tsdf_walk.hpp: AccOut::seg_ticket, place_segment, seg_place, runs_count): the walk's count of
a chunk's segments returns every segment's index among them, and the segment descriptors reach chunk order by that index —
in an order that differs from run to run.  The apply stage adds fixed-point sums and takes maxima, so the maps must not.

The scenes (tests/segment_tickets_scenario.py) run once per setting of PLVS_TSDF_COLLECT, each in a process of its own: the
switch and the trace are read once per process.  2: runs_count places the segments of every call that is not launched on
predicted sizes; 0: seg_place places them all.  Tolerances: those of tests/test_tsdf_chisel.py for the order-free mode."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_tsdf_chisel import ORDER_FREE_SDF_ATOL, ORDER_FREE_WEIGHT_RTOL, small_cam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INITIAL_SEG_SPILL = 1 << 12    # segments / records of spill room a fresh handle starts with (walk_scratch)
INITIAL_REC_SPILL = 1 << 16


def _run(mode):
    env = dict(os.environ, PLVS_TSDF_COLLECT=str(mode), PLVS_HIP_TSDF_TRACE="1")
    p = subprocess.run([sys.executable, "-m", "tests.segment_tickets_scenario"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    scenes = {}
    for ln in p.stdout.splitlines():
        if ln.startswith("{"):
            rec = json.loads(ln)
            scenes[rec["scene"]] = rec
    traces, name = {}, None
    for ln in p.stderr.splitlines():
        if ln.startswith("[scene] "):
            name = ln.split()[1]
        elif "[tsdf_chisel] tiles" in ln and name is not None:
            t = ln[ln.index("[tsdf_chisel] tiles"):]
            traces.setdefault(name, []).append({k: int(v) for k, v in re.findall(r"(\w+) (-?\d+)", t)})
    return scenes, traces


@pytest.fixture(scope="module")
def collected():
    return _run(2)


@pytest.fixture(scope="module")
def plain():
    return _run(0)


def _within_tolerance(rec):
    o = rec["oracle"]
    print("%s: %d chunks, sdf %.3g m, weight %.3g rel" % (rec["scene"], o["chunks"], o["sdf"], o["weight"]))
    assert o["same_chunks"] and o["chunks"] > 0
    assert o["exact"], "kfid, colour and the observed set are exact"
    assert o["sdf"] <= ORDER_FREE_SDF_ATOL and o["weight"] <= ORDER_FREE_WEIGHT_RTOL


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["small_1", "small_5"])
def test_hip_small_calls_place_their_segments_by_ticket(collected, plain, scene):
    for scenes, traces in (collected, plain):
        _within_tolerance(scenes[scene])
        assert traces[scene][-1]["tiles"] == 40 * (1 if scene == "small_1" else 5)
    assert all(t["chain"] != 2 for t in plain[1][scene]), "seg_place's path: no collected chain"


@pytest.mark.gpu
def test_hip_collected_chain_on_and_off_leave_the_same_maps(collected, plain):
    assert set(collected[0]) == set(plain[0]) and len(plain[0]) == 11
    for name in sorted(plain[0]):
        a, b = collected[0][name], plain[0][name]
        assert a["map"] == b["map"] and a["updated"] == b["updated"] and a["stats"] == b["stats"], name
        if a["oracle"] is not None:
            _within_tolerance(a)
            _within_tolerance(b)
    chains = [t["chain"] for ts in collected[1].values() for t in ts]
    assert chains.count(2) >= 3, chains                       # runs_count placed, the collected chain folded
    assert all(t["chain"] != 2 for ts in plain[1].values() for t in ts)


@pytest.mark.gpu
def test_hip_busy_chunk_applied_in_parts(collected, plain):
    for scenes, traces in (collected, plain):
        t = traces["busy"][-1]
        assert t["tiles"] == 750 and t["multi"] >= 1 and t["parts"] > t["updated"], t
        _within_tolerance(scenes["busy"])


@pytest.mark.gpu
def test_hip_tiles_of_the_general_kernel_take_tickets(collected, plain):
    for scenes, traces in (collected, plain):
        t = traces["general"][-1]
        assert t["seg_top"] > 0, "segments in the spill area: written by walk_tiles alone"
        assert t["chain"] != 2, "a call with a tile left to walk_tiles is not the collected chain's"
        _within_tolerance(scenes["general"])


@pytest.mark.gpu
def test_hip_scratch_retry_leaves_no_ticket_behind(collected, plain):
    for scenes, traces in (collected, plain):
        t, rec = traces["retry"][-1], scenes["retry"]
        assert t["seg_top"] > INITIAL_SEG_SPILL or t["rec_top"] > INITIAL_REC_SPILL, "the first attempt must run out of scratch"
        _within_tolerance(rec)
        assert rec["updated_chunks"] == rec["oracle_chunks"] and rec["n_updated"] == rec["stats"]["updated_chunks"]


@pytest.mark.gpu
def test_hip_repeated_calls_are_bit_identical(collected, plain):
    for scenes, _ in (collected, plain):
        for i in range(3):
            a, b = scenes[f"repeat_0_{i}"], scenes[f"repeat_1_{i}"]
            assert a["stats"]["visits"] > 0 and a["n_updated"] > 0
            assert a["map"] == b["map"] and a["updated"] == b["updated"] and a["stats"] == b["stats"], i


@pytest.mark.gpu
def test_hip_ray_sharded_integrate_at_one_rank_equals_the_order_free_map():
    """The received segments of the ray-sharded integrate carry no tickets: its own counting sort (seg_pass) places them."""
    from plvs_amd.tsdf import TsdfChisel
    from tests.synth_scene import make_keyframes
    from tests.test_shard_rays import _batch, sharded_step
    kfs = make_keyframes(4, cam=small_cam(2), seed=17)
    single = TsdfChisel(0.05, max_chunks=4096, order_free=True)
    rank = TsdfChisel(0.05, max_chunks=4096, shard_rank=0, shard_count=1, order_free=True)
    for part in (kfs[:3], kfs[3:]):
        xyz, rgb, kfid, offsets, Twc = _batch(part)
        single.integrate_batch_dev(xyz, rgb, kfid, offsets, Twc)
        sharded_step([rank], xyz, rgb, kfid, offsets, Twc)
        assert rank.last_stats()["visits"] == single.last_stats()["visits"] > 0
    ids = {tuple(x) for x in single.chunk_ids()}
    assert ids == {tuple(x) for x in rank.chunk_ids()} and len(ids) > 4
    for cid in sorted(ids):
        for x, y in zip(single.get_chunk(*cid), rank.get_chunk(*cid)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"chunk {cid} differs"
    single.close()
    rank.close()
