"""Per-stage timing of the chisel back end (set_profiling / stage_ms): the contract bench.py reads, for each of the
three pipelines that record stage events — ordered, order-free, and the owner's side of the ray-sharded integrate.

After one call with profiling on: the stage names of the pipeline (6 ordered, 4 of the walk), calls == 1, every time
finite and >= 0, and > 0 for the stages that ran.  The one stage that does not run: walk_tiles of shard_apply — the walk
ran in shard_walk, its two events are recorded back to back.  (fold_colours of an order-free call is "what the colour fold
adds behind the apply stage"; on a handle's first call the fold is launched only after the host has read the walk's
counters, behind an apply stage queued before that read, so it adds time.)
"""
import math

import numpy as np
import pytest
import torch

from tests.synth_scene import make_keyframes
from tests.test_shard_rays import _batch, send_buffers, virtual_all_to_all

ORDERED = ["ray_count", "scan", "ray_tiles", "sort_runs", "gather_runs", "chain_runs"]
WALK = ["walk_tiles", "sort_segments", "apply_chunks", "fold_colours"]


def _check(t, names, ran):
    ms, calls = t.stage_ms()
    print(f"stage_ms after one call: {ms} calls {calls}")
    assert list(ms) == names
    assert calls == 1
    for name, v in ms.items():
        assert math.isfinite(v) and v >= 0.0, f"{name}: {v}"
    for name in ran:
        assert ms[name] > 0.0, f"{name} ran and took no time"


@pytest.mark.gpu
def test_stage_times_of_one_call_of_each_pipeline():
    from plvs_amd.tsdf import TsdfChisel
    xyz, rgb, kfid, offsets, Twc = _batch(make_keyframes(2, seed=5))

    ordered = TsdfChisel(0.05, max_chunks=2048)
    ordered.set_profiling(True)
    assert ordered.stage_ms() == ({n: 0.0 for n in ORDERED}, 0)
    ordered.integrate_batch_dev(xyz, rgb, kfid, offsets, Twc)
    torch.cuda.synchronize()
    assert ordered.last_stats()["visits"] > 0
    _check(ordered, ORDERED, ORDERED)
    ordered.close()

    free = TsdfChisel(0.05, max_chunks=2048, order_free=True)
    free.set_profiling(True)
    free.integrate_batch_dev(xyz, rgb, kfid, offsets, Twc)
    torch.cuda.synchronize()
    assert free.last_stats()["visits"] > 0
    _check(free, WALK, WALK)
    free.close()

    rank = TsdfChisel(0.05, max_chunks=2048, shard_rank=0, shard_count=1, order_free=True)
    rank.set_profiling(True)
    counts = [rank.shard_walk(xyz, offsets, Twc)]
    bufs = [send_buffers(rank, counts[0])]
    torch.cuda.synchronize()
    (seg, rec, run, rc), = virtual_all_to_all(counts, bufs)
    assert rc[0, 0] > 0 and rc[0, 2] > 0, "descriptors and colour runs to apply"
    rank.shard_apply(seg, rec, run, rc, rgb, kfid)
    torch.cuda.synchronize()
    assert rank.last_stats()["visits"] > 0
    _check(rank, WALK, WALK[1:])
    rank.close()
