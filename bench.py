#!/usr/bin/env python3
"""bench.py — the driver's measurement contract.

  python bench.py --gpus N --steps K --warmup W          (N = 1)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Metric (BASELINE.json): Mvoxels/s of TSDF integrate (voxel read-modify-write
visits per second), config "Chisel TSDF 5 cm / 5 m, 640x480 RGB-D" on a seeded
synthetic room.  One *step* = one call of
plvs_hip_tsdf_chisel_integrate_batch_dev over a batch of `--batch` keyframes
(76 800 camera-frame points each) that are already resident in HBM.

`value` is the order-free mode — what BASELINE's north star asks of the TSDF:
sdf / weight within a stated float tolerance (tests/test_tsdf_chisel.py: 2e-5 m,
5e-5 relative; deterministic: the sums are fixed point), kfid and colour exact.
The bit-exact ordered mode is measured beside it (`bit_exact_mode`; `--ordered`
makes it the headline).  After the timed loops the final maps of both modes are
compared with the CPU oracle run over the very same sequence (`parity_checked`);
that oracle run is also the `cpu_baseline`.

Multi-GPU (N > 1): the voxel-chunk hash is sharded, owner(chunk) =
ChunkHasher(id) mod N, and the RAYS are sharded by tile of the point stream
(plvs_amd/csrc/tsdf_shard.hpp): rank r walks tiles t = r (mod N), its partial
sums and colour runs travel to the chunk owners in one all-to-all per step, the
per-step lists of updated chunk ids and of newly colour-saturated voxels are
all-gathered — all over RCCL.  The union of the shards is bit-identical to the
single-GPU order-free map (tests/test_shard_rays.py).  Weak scaling: a step
carries --batch keyframes per GPU (--strong keeps the step fixed).  The ordered
mode and the voxblox back end keep the chunk-hash shard with replicated walks;
BASELINE's configs[3] (voxblox 2 cm, 16x12x3 m room) is measured at every N as
the `voxblox_configs3` leg.

The JSON line also carries `roofline` (algorithmic bytes of SURVEY §8d over the
measured GPU time of the integrate pipeline, per-stage times from HIP events on
the library's own stream, HBM traffic from the committed PMC passes) and under
"frontend" the per-frame front end — N = 1 only.

A plain run sets up, warms up, times the --steps steps and prints the line.
Everything else — the other chisel mode, the steady-state, first-lap and
UpdateMap-sized legs, the parity check against the oracle and the CPU
baselines, the voxblox configs[3] leg, the front end, the per-phase times and
the other scaling rule of N > 1 — runs with --full (the --no-* switches turn
single legs of such a run off), which also writes the full result to
bench_out/bench_full.json.  --dump-outputs DIR writes what the last timed step
left for its caller (stats, updated chunk ids, their voxels) as .npy files.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=100,
                    help="keyframes per step (default: the whole 100-pose sequence of SURVEY §8d in one launch)")
    ap.add_argument("--resolution", type=float, default=0.05)
    ap.add_argument("--max-depth", type=float, default=5.0)
    ap.add_argument("--backend", choices=["chisel", "voxblox"], default="chisel",
                    help="chisel = configs[2] (5 cm / 5 m); voxblox = configs[3] stand-in (2 cm / 8 m room)")
    ap.add_argument("--ordered", action="store_true",
                    help="chisel: make the bit-exact ordered mode the headline (default: the order-free mode, sdf / "
                         "weight within the float tolerance stated in tests/test_tsdf_chisel.py; kfid, colour exact)")
    ap.add_argument("--order-free", action="store_true", help="(the default; kept for older command lines)")
    ap.add_argument("--no-other-mode-leg", action="store_true", help="skip the measurement of the other chisel mode")
    ap.add_argument("--no-voxblox-leg", action="store_true", help="skip the configs[3] (voxblox 2 cm) leg")
    ap.add_argument("--sharded-at-one", action="store_true",
                    help="N = 1: run the step through the multi-GPU code path (a process group of one rank), to exercise it")
    ap.add_argument("--strong", action="store_true",
                    help="N > 1: keep the step at --batch keyframes (default: --batch keyframes per GPU, weak scaling)")
    ap.add_argument("--no-parity-check", action="store_true",
                    help="skip the oracle run over the same sequence (parity check + CPU baseline)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-realistic-legs", action="store_true", help="skip the first-lap and 5- / 1-key-frame-call legs")
    ap.add_argument("--steady-state", action="store_true",
                    help="chisel: make the saturated-map workload of rounds 1-3 the headline (every step re-integrates the same "
                         "100 key frames of the small room); default: the long trajectory of distinct key frames")
    ap.add_argument("--no-steady-state-leg", action="store_true", help="skip the saturated-map leg beside the headline")
    ap.add_argument("--no-frontend", action="store_true")
    ap.add_argument("--cloud-input", action="store_true",
                    help="chisel, N = 1, order-free: feed the steps as point streams (plvs_hip_tsdf_chisel_integrate_batch_dev, the "
                         "headline of rounds 1-4) instead of as the depth images the clouds are made from "
                         "(plvs_hip_tsdf_chisel_integrate_depth_batch_dev: GeneratePointCloudInCameraFrameBGRA + InsertCloud in one "
                         "call, the default since round 5)")
    ap.add_argument("--verbose-line", action="store_true",
                    help="print the full result (every leg with its prose) instead of the compact line; a --full run also "
                         "writes the full result to bench_out/bench_full.json")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, run every other leg (other chisel mode, steady state, first lap and "
                         "UpdateMap-sized calls, parity check and CPU baselines, voxblox configs[3], front end; at N > 1 the "
                         "per-phase times and the other scaling rule); default: the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step left for its caller as DIR/<name>.npy "
                         "(float32 / float64): its stats, the ids of the chunks it updated and their voxels (a fixed, seeded "
                         f"sample of {DUMP_MAX_CHUNKS} chunks where it updated more)")
    return ap.parse_args()


DUMP_MAX_CHUNKS = 512      # 512 chunks x 4096 voxels x 24 B: 50 MB of voxels, within the 64 MB of a dump


def dump_outputs(tsdf, out_dir, stats, vbx):
    """--dump-outputs: the arrays a caller of the timed path receives after its last step — last_stats(), the sorted ids of
    the chunks (voxblox: blocks) the step updated, and those chunks' voxels as get_chunk() downloads them (every chunk, or
    a sample of DUMP_MAX_CHUNKS drawn with a fixed seed).  Integers go out as float64 (exact), sdf / weight as float32."""
    os.makedirs(out_dir, exist_ok=True)
    keys = ("visits", "points", "new_chunks", "updated_chunks", "voxels", "max_run")
    np.save(os.path.join(out_dir, "last_step_stats.npy"), np.array([stats[k] for k in keys], np.float64))
    ids = tsdf.updated_chunk_ids()
    ids = ids[np.lexsort(ids.T[::-1])] if len(ids) else ids.reshape(0, 3)
    np.save(os.path.join(out_dir, "updated_chunk_ids.npy"), ids.astype(np.float64))
    pick = np.arange(len(ids))
    if len(ids) > DUMP_MAX_CHUNKS:
        pick = np.sort(np.random.default_rng(0).choice(len(ids), DUMP_MAX_CHUNKS, replace=False))
    np.save(os.path.join(out_dir, "dumped_chunk_ids.npy"), ids[pick].astype(np.float64))
    names = ("distance", "weight", "rgba") if vbx else ("sdf", "weight", "kfid", "colour")
    cols = [[] for _ in names]
    for cid in ids[pick]:
        for c, a in zip(cols, tsdf.get_chunk(*cid)):
            c.append(a)
    for name, c in zip(names, cols):
        a = np.stack(c) if c else np.zeros((0, 4096))
        np.save(os.path.join(out_dir, f"chunk_{name}.npy"), a if a.dtype == np.float32 else a.astype(np.float64))


def compact_line(r):
    """The one JSON line of the driver's contract, numbers only (round 5).  The full result of a --full run — every leg with
    the prose that says what it is — goes to bench_out/bench_full.json and is described in DESIGN.md §4.6; the driver keeps
    the contract keys, the scalar members of `config`, `roofline` and `cpu_baseline`, and the last 2 KB of the line, so the
    key figures of every leg are lifted into those three objects as flat scalars and repeated in `summary`, the LAST key of
    the line."""
    def g(d, *path, default=None):
        for k in path:
            if not isinstance(d, dict) or k not in d:
                return default
            d = d[k]
        return d

    def short(x, n=110):
        return x if not isinstance(x, str) or len(x) <= n else x[:n - 1] + "~"
    out = {k: r[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                             "vs_baseline", "dtype", "data") if k in r}
    cfg = dict(r.get("config", {}))
    wl = cfg.get("workload", "")
    cfg["workload"] = (wl.split(":")[0] + ": see DESIGN.md 4.1 / 4.6") if len(wl) > 110 else wl
    cfg = {k: short(v) for k, v in cfg.items() if not isinstance(v, (dict, list)) or k == "ms_per_step_median_max"}
    roof = {k: short(v) for k, v in r.get("roofline", {}).items() if not isinstance(v, dict)}
    for k, v in (g(r, "roofline", "stage_ms_per_launch", default={}) or {}).items():
        roof["ms_" + k] = v
    cpu = {k: short(v, 160) for k, v in r.get("cpu_baseline", {}).items() if not isinstance(v, dict)}
    summary = {
        "frac": g(r, "roofline", "frac"), "ms_gpu": g(r, "roofline", "ms_per_launch"),
        "steady_state_value": g(r, "steady_state", "value"), "steady_state_frac": g(r, "steady_state", "roofline", "frac"),
        "steady_state_ms": g(r, "steady_state", "roofline", "ms_per_launch"),
        "bit_exact_value": g(r, "bit_exact_mode", "value"), "bit_exact_frac": g(r, "bit_exact_mode", "roofline", "frac"),
        "bit_exact_ms": g(r, "bit_exact_mode", "roofline", "ms_per_launch"),
        "first_lap_ms": g(r, "realistic_legs", "first_lap", "ms_per_call"),
        "updatemap_5_ms": g(r, "realistic_legs", "updatemap_5", "second_lap", "ms_per_call_median"),
        "updatemap_1_ms": g(r, "realistic_legs", "updatemap_1", "second_lap", "ms_per_call_median"),
        "updatemap_1_frac": g(r, "realistic_legs", "updatemap_1", "second_lap", "roofline_frac"),
        "voxblox_value": g(r, "voxblox_configs3", "value"), "voxblox_ms": g(r, "voxblox_configs3", "ms_per_step"),
        "voxblox_frac": g(r, "voxblox_configs3", "roofline", "frac"), "voxblox_traffic": g(r, "voxblox_configs3", "roofline", "traffic"),
        "voxblox_cpu_value": g(r, "voxblox_configs3", "cpu_baseline", "value"),
        "voxblox_cpu_kind": g(r, "voxblox_configs3", "cpu_baseline", "kind"),
        "voxblox_fast_ms_per_kf": g(r, "voxblox_configs3", "fast_method", "hip_ms_per_keyframe"),
        "voxblox_fast_bit_identical": g(r, "voxblox_configs3", "fast_method", "bit_identical_to_the_reference_layer"),
        "frontend_ms_per_frame": g(r, "frontend", "ms_per_frame"), "frontend_fps": g(r, "frontend", "frames_per_s"),
        "frontend_orb_ms": g(r, "frontend", "orb_extract_ms"), "frontend_lines_ms": g(r, "frontend", "lines_extract_ms"),
        "frontend_cpu_ms_per_frame": g(r, "frontend", "cpu_baseline", "ms_per_frame"),
        "frontend_cpu_kind": g(r, "frontend", "cpu_baseline", "kind"),
        "lsd_ms_per_frame": g(r, "frontend", "lsd_extract", "ms_per_frame"),
        "lsd_cpu_ms_per_frame": g(r, "frontend", "lsd_extract", "cpu_baseline", "ms_per_frame"),
        "lsd_parity_ok": g(r, "frontend", "lsd_extract", "parity_ok"),
        "sgm_ms_per_pair_parity_unpinned": g(r, "frontend", "dense_stereo_sgm", "ms_per_pair"),
        "sgm_parity": "unpinned (libsgm is CUDA-only, not compilable here: oracle/sgm.c is a restatement nothing checks)" if g(r, "frontend", "dense_stereo_sgm") else None,
        "elas_parity_note": "bit-identical on zero-initialised heaps (oracle/ref/elas_zero_malloc.h)" if g(r, "kitti_shaped", "ms_per_keyframe") else None,
        "kitti_ms_per_keyframe_incl_reference_host_stages": g(r, "kitti_shaped", "ms_per_keyframe"),
        "kitti_note": ("NOT a product number: libelas' host stages (support filters, Delaunay, planes, grid) run inside the "
                       "reference's compiled Elas::process (oracle/_ref/libelas_ref.so); the device stages are the product's")
        if g(r, "kitti_shaped", "ms_per_keyframe") else None,
        "kitti_maps_bit_identical": g(r, "kitti_shaped", "disparity_maps_bit_identical_to_reference"),
        "parity_ok": r.get("parity_checked"),
        "parity_bit_exact_mode": g(r, "parity", "bit_exact_mode", "sdf_weight"),
        "parity_order_free_worst_fraction_of_bound_sdf": g(r, "parity", "order_free_mode",
                                                           "order_free_vs_reference_f32_worst_fraction_of_bound", "sdf"),
        "parity_order_free_worst_fraction_of_bound_weight": g(r, "parity", "order_free_mode",
                                                              "order_free_vs_reference_f32_worst_fraction_of_bound", "weight"),
        "parity_order_free_vs_exact_mean_sdf_m": g(r, "parity", "order_free_mode", "order_free_vs_exact_mean", "max_abs_sdf_m"),
        "parity_chunks": g(r, "parity", "order_free_mode", "chunks"),
    }
    summary = {k: v for k, v in summary.items() if v is not None}
    # the lifted copies (the driver's record keeps scalars of these three objects)
    for k in ("steady_state_frac", "steady_state_value", "bit_exact_frac", "bit_exact_value", "voxblox_frac", "voxblox_value",
              "voxblox_traffic"):
        if k in summary:
            roof[k] = summary[k]
    for k in ("first_lap_ms", "updatemap_5_ms", "updatemap_1_ms", "frontend_ms_per_frame", "lsd_ms_per_frame",
              "kitti_ms_per_keyframe_incl_reference_host_stages", "parity_ok"):
        if k in summary:
            cfg[k] = summary[k]
    for k in ("voxblox_cpu_value", "frontend_cpu_ms_per_frame", "lsd_cpu_ms_per_frame"):
        if k in summary:
            cpu[k] = summary[k]
    out["config"], out["roofline"], out["cpu_baseline"] = cfg, roof, cpu
    for k in ("phases_ms", "other_scaling_leg"):
        if k in r:
            out[k] = r[k]
    if r.get("legs_present") is not None:
        out["full_result"] = "bench_out/bench_full.json (every leg of a --full run; a run with legs switched off: bench_partial.json)"
    out["summary"] = summary
    return out


def leg_realistic_calls(C):
    # ------------------------------------------------- what PLVS runs, not only the steady state (N = 1 only)
    # (main's locals this leg reads)
    TsdfChisel = getattr(C, 'TsdfChisel', None)
    args = getattr(C, 'args', None)
    batches = getattr(C, 'batches', None)
    k = getattr(C, 'k', None)
    kfs = getattr(C, 'kfs', None)
    multi = getattr(C, 'multi', None)
    n_poses = getattr(C, 'n_poses', None)
    rank = getattr(C, 'rank', None)
    result = getattr(C, 'result', None)
    sel = getattr(C, 'sel', None)
    st = getattr(C, 'st', None)
    t = getattr(C, 't', None)
    t0 = getattr(C, 't0', None)
    vbx = getattr(C, 'vbx', None)
    world = getattr(C, 'world', None)
    # The headline step re-integrates the same 100 key frames into a map that has seen them: no chunk is allocated,
    # nearly every colour has saturated.  Two legs with the rest inside the timed region:
    #  first_lap    a FRESH map takes the 100 key frames in one call: chunk allocation, directory inserts, a run and a
    #               colour fold for every voxel (all below weight 254)
    #  updatemap_5  the same stream in calls of 5 key frames — what PointCloudMapping::UpdateMap hands over
    #               (src/PointCloudMapping.cc:552) — on a fresh map (first lap) and on the map that lap left (second lap)
    if rank == 0 and world == 1 and not vbx and not multi and not args.no_realistic_legs:
        tl = TsdfChisel(args.resolution, max_chunks=16384, order_free=not args.ordered)
        b0 = batches[0]

        def timed_call(t, b):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.integrate_batch_dev(*b)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, t.last_stats()

        laps = []
        for rep in range(4):          # (the first repetition also sizes the handle's scratch buffers: dropped)
            tl.clear()
            dt, st = timed_call(tl, b0)
            laps.append((dt, st))
        dt = float(np.median([x[0] for x in laps[1:]]))
        st = laps[-1][1]
        legs = {"first_lap": {
            "what": "one call of 100 key frames into an EMPTY map (median of 3 calls, each on a cleared map)",
            "ms_per_call": round(dt * 1e3, 3), "value": round(st["visits"] / dt / 1e6, 2), "unit": "Mvoxels/s",
            "new_chunks": st["new_chunks"], "voxels": st["voxels"],
            "roofline_frac": round((32.0 * st["visits"] + 28.0 * st["points"]) / dt / 8e12, 5)}}
        sel = [kfs[j % n_poses] for j in range(100)]
        small = []
        for j0 in range(0, 100, 5):
            grp = sel[j0:j0 + 5]
            small.append((torch.from_numpy(np.concatenate([k["xyz"] for k in grp])).cuda(),
                          torch.from_numpy(np.concatenate([k["rgb"] for k in grp])).cuda(),
                          torch.from_numpy(np.concatenate([k["kfid"] for k in grp]).astype(np.int32)).cuda(),
                          np.cumsum([0] + [k["xyz"].shape[0] for k in grp]).astype(np.int32),
                          torch.from_numpy(np.stack([k["Twc"] for k in grp])).cuda()))
        for lap_name in ("warm-up", "first_lap", "second_lap"):
            if lap_name != "second_lap":
                tl.clear()
            ts, vs = [], 0
            for b in small:
                dtc, stc = timed_call(tl, b)
                ts.append(dtc)
                vs += stc["visits"]
            if lap_name != "warm-up":
                legs.setdefault("updatemap_5", {"what": "20 calls of 5 key frames each (PointCloudMapping::UpdateMap's batch)"})[lap_name] = {
                    "ms_per_call_median": round(float(np.median(ts)) * 1e3, 4), "ms_per_call_max": round(max(ts) * 1e3, 4),
                    "value": round(vs / sum(ts) / 1e6, 2), "unit": "Mvoxels/s"}
        # updatemap_1: ONE key frame per call — PLVS's real call shape: PointCloudMapChisel::InsertCloud per key frame
        # (src/PointCloudMapping.cc:540, src/PointCloudMapChisel.cc:76)
        one = []
        for k in sel[:40]:
            one.append((torch.from_numpy(k["xyz"]).cuda(), torch.from_numpy(k["rgb"]).cuda(),
                        torch.from_numpy(k["kfid"].astype(np.int32)).cuda(),
                        np.array([0, k["xyz"].shape[0]], np.int32), torch.from_numpy(k["Twc"][None]).cuda()))
        for lap_name in ("warm-up", "first_lap", "second_lap"):
            if lap_name != "second_lap":
                tl.clear()
            ts, vs = [], 0
            for b in one:
                dtc, stc = timed_call(tl, b)
                ts.append(dtc)
                vs += stc["visits"]
            if lap_name != "warm-up":
                legs.setdefault("updatemap_1", {"what": "40 calls of ONE key frame each (PointCloudMapChisel::InsertCloud per key frame)"})[lap_name] = {
                    "ms_per_call_median": round(float(np.median(ts)) * 1e3, 4), "ms_per_call_max": round(max(ts) * 1e3, 4),
                    "value": round(vs / sum(ts) / 1e6, 2), "unit": "Mvoxels/s",
                    "roofline_frac": round((32.0 * vs + 28.0 * sum(int(b[3][1]) for b in one)) / sum(ts) / 8e12, 5)}
        tl.close()
        result["realistic_legs"] = legs


def leg_steady_state(C):
    # ------------------------------------------------- the saturated-map workload of rounds 1-3, beside the headline
    # (main's locals this leg reads)
    TsdfChisel = getattr(C, 'TsdfChisel', None)
    args = getattr(C, 'args', None)
    depth_input = getattr(C, 'depth_input', None)
    k = getattr(C, 'k', None)
    make_keyframes = getattr(C, 'make_keyframes', None)
    multi = getattr(C, 'multi', None)
    pack_depth = getattr(C, 'pack_depth', None)
    rank = getattr(C, 'rank', None)
    result = getattr(C, 'result', None)
    t0 = getattr(C, 't0', None)
    v = getattr(C, 'v', None)
    vbx = getattr(C, 'vbx', None)
    world = getattr(C, 'world', None)
    if rank == 0 and world == 1 and not vbx and not multi and not args.steady_state and not args.no_steady_state_leg:
        sk = make_keyframes(100, max_depth=args.max_depth, seed=0, images=depth_input)
        if depth_input:
            sb = pack_depth(sk)
            spts = sum(k["xyz"].shape[0] for k in sk)
            s_call = lambda: ts_.integrate_depth_batch_dev(*sb)   # noqa: E731
        else:
            sb = (torch.from_numpy(np.concatenate([k["xyz"] for k in sk])).cuda(),
                  torch.from_numpy(np.concatenate([k["rgb"] for k in sk])).cuda(),
                  torch.from_numpy(np.concatenate([k["kfid"] for k in sk]).astype(np.int32)).cuda(),
                  np.cumsum([0] + [k["xyz"].shape[0] for k in sk]).astype(np.int32),
                  torch.from_numpy(np.stack([k["Twc"] for k in sk])).cuda())
            spts = int(sb[3][-1])
            s_call = lambda: ts_.integrate_batch_dev(*sb)         # noqa: E731
        ts_ = TsdfChisel(args.resolution, max_chunks=16384, order_free=not args.ordered)
        for _ in range(10):
            s_call()
        torch.cuda.synchronize()
        ts_.set_profiling(True)
        t0 = time.perf_counter()
        sv = sp = 0
        for _ in range(10):
            s_call()
            st_ = ts_.last_stats()
            sv += st_["visits"]
            sp += spts
        torch.cuda.synchronize()
        sel_ = time.perf_counter() - t0
        ssm, sc = ts_.stage_ms()
        ts_.set_profiling(False)
        ts_.close()
        sms = sum(ssm.values())
        result["steady_state"] = {
            "what": "rounds 1-3's headline workload: the same 100 key frames (room 6x4x3 m, camera circle r=1 m, 76800 points "
                    "each) re-integrated into a map that has seen them 10 times — no chunk allocation, colours saturated, "
                    "inputs and map resident in the Infinity Cache (10 warm-up + 10 timed steps)",
            "value": round(sv / sel_ / 1e6, 2), "unit": "Mvoxels/s", "ms_per_step": round(sel_ / 10 * 1e3, 3),
            "visits_per_step": int(sv // 10),
            "stage_ms_per_launch": {n: round(v / max(sc, 1), 4) for n, v in ssm.items()},
            "roofline": {"bound": "hbm", "achieved": round((32.0 * sv + 28.0 * sp) / (sms * 1e-3) / 1e9, 2), "peak": 8000.0,
                         "unit": "GB/s", "frac": round((32.0 * sv + 28.0 * sp) / (sms * 1e-3) / 1e9 / 8000.0, 5),
                         "ms_per_launch": round(sms / max(sc, 1), 4)}}


def leg_other_chisel_mode(C):
    # ------------------------------------------------- the other chisel mode, same stream (N = 1 only)
    # (main's locals this leg reads)
    TsdfChisel = getattr(C, 'TsdfChisel', None)
    args = getattr(C, 'args', None)
    batches = getattr(C, 'batches', None)
    rank = getattr(C, 'rank', None)
    result = getattr(C, 'result', None)
    s = getattr(C, 's', None)
    t0 = getattr(C, 't0', None)
    total_steps = getattr(C, 'total_steps', None)
    v = getattr(C, 'v', None)
    vbx = getattr(C, 'vbx', None)
    world = getattr(C, 'world', None)
    t2 = None
    if rank == 0 and world == 1 and not vbx and not args.no_other_mode_leg:
        t2 = TsdfChisel(args.resolution, max_chunks=16384, order_free=args.ordered)
        for s in range(args.warmup):
            t2.integrate_batch_dev(*[batches[s][i] for i in (0, 1, 2, 3, 4)])
        torch.cuda.synchronize()
        t2.set_profiling(True)
        t0 = time.perf_counter()
        v2 = p2 = 0
        for s in range(args.warmup, total_steps):
            t2.integrate_batch_dev(*[batches[s][i] for i in (0, 1, 2, 3, 4)])
            st2 = t2.last_stats()
            v2 += st2["visits"]
            p2 += st2["points"]
        torch.cuda.synchronize()
        el2 = time.perf_counter() - t0
        sm2, c2 = t2.stage_ms()
        t2.set_profiling(False)
        ms2 = sum(sm2.values())
        ach2 = (32.0 * v2 + 28.0 * p2) / (ms2 * 1e-3) / 1e9 if ms2 > 0 else 0.0
        leg = {
            "value": round(v2 / el2 / 1e6, 2), "unit": "Mvoxels/s", "ms_per_step": round(el2 / args.steps * 1e3, 3),
            "stage_ms_per_launch": {n: round(v / max(c2, 1), 4) for n, v in sm2.items()},
            "roofline": {"bound": "hbm", "achieved": round(ach2, 2), "peak": 8000.0, "unit": "GB/s",
                         "frac": round(ach2 / 8000.0, 5), "ms_per_launch": round(ms2 / max(c2, 1), 4)},
        }
        if args.ordered:
            leg["what"] = ("plvs_tsdf_chisel_params.order_free = 1: one walk; the visits of a call are summed per voxel "
                           "in fixed point (per tile in LDS, then per chunk slab in LDS) and applied in one update")
            result["order_free_mode"] = leg
        else:
            leg["what"] = ("plvs_tsdf_chisel_params.order_free = 0: every voxel update applied in the reference's order "
                           "(count, scan, tile sort, run sort, gather, sequential chain); sdf / weight bit-identical")
            result["bit_exact_mode"] = leg
    # (what the rest of main reads again)
    _l = locals()
    if 't2' in _l:
        C.t2 = _l['t2']


def leg_parity_and_cpu_baseline(C):
    # ------------------------------------------------- parity of the timed maps + CPU baseline (rank 0, N = 1)
    # (main's locals this leg reads)
    args = getattr(C, 'args', None)
    b = getattr(C, 'b', None)
    k = getattr(C, 'k', None)
    kfs = getattr(C, 'kfs', None)
    n_poses = getattr(C, 'n_poses', None)
    rank = getattr(C, 'rank', None)
    result = getattr(C, 'result', None)
    s = getattr(C, 's', None)
    t0 = getattr(C, 't0', None)
    t2 = getattr(C, 't2', None)
    total_steps = getattr(C, 'total_steps', None)
    tsdf = getattr(C, 'tsdf', None)
    vbx = getattr(C, 'vbx', None)
    world = getattr(C, 'world', None)
    if rank == 0 and world == 1 and not vbx and not args.no_parity_check and not args.no_cpu_baseline:
        from tests import oracle_lib
        oracle = oracle_lib.load()
        ora = oracle.chisel(args.resolution)
        ora.track_exact()   # the exact (double) mean of the same visits beside the reference's f32 running mean
        t0 = time.perf_counter()
        cv = 0
        for s in range(total_steps):
            for j in range(args.batch):
                k = kfs[(s * args.batch + j) % n_poses]
                ora.integrate(k["xyz"], k["rgb"], k["kfid"], k["Twc"])
                cv += ora.last_visits()
        ct = time.perf_counter() - t0
        port = {
            "value": round(cv / ct / 1e6, 3), "unit": "Mvoxels/s", "cores": 1, "kind": "port",
            "sample": f"oracle/tsdf_chisel.c (the reference's sequential loop, gcc -O3 -march=x86-64-v3 -ffp-contract=off, "
                      f"with the exact-mean accumulators of the parity check on) over the same "
                      f"{total_steps * args.batch} keyframes the device integrated, {ct:.1f} s, host has {os.cpu_count()} cores",
        }
        result["cpu_baseline"] = port
        # ... and the reference ITSELF where its compiled library travelled with the snapshot: all of open_chisel built
        # unmodified with the reference's flags (oracle/ref/Makefile -> oracle/_ref/libchisel_full_ref_o3.so), on a
        # bounded sample of the same stream (the reference integrates one voxel per unordered_map look-up)
        ref_so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracle", "_ref", "libchisel_full_ref_o3.so")
        if os.path.exists(ref_so):
            import tests.test_oracle_pinned_chisel_map as pinned
            pinned.REF = ref_so
            from tests.synth_scene import TUM1
            refmap = pinned.RefChisel(args.resolution, dict(TUM1))
            nref = min(total_steps * args.batch, 120)
            for j in range(5):
                k = kfs[j % n_poses]
                refmap.integrate(k["xyz"], k["rgb"], k["kfid"], k["Twc"])
            t0 = time.perf_counter()
            rv = 0
            for j in range(nref):
                k = kfs[(5 + j) % n_poses]
                refmap.integrate(k["xyz"], k["rgb"], k["kfid"], k["Twc"])
            rt = time.perf_counter() - t0
            # (the reference exposes no visit counter: the visits of the same keyframes as the port counted them)
            probe = oracle.chisel(args.resolution)
            for j in range(nref):
                k = kfs[(5 + j) % n_poses]
                probe.integrate(k["xyz"], k["rgb"], k["kfid"], k["Twc"])
                rv += probe.last_visits()
            probe.close()
            refmap.close()
            result["cpu_baseline"] = {
                "value": round(rv / rt / 1e6, 3), "unit": "Mvoxels/s", "cores": 1, "kind": "reference",
                "sample": f"chisel::Chisel::IntegratePointCloudWidthDepth of the reference's own open_chisel sources (g++ -O3 "
                          f"-march=x86-64-v3 as its CMakeLists asks, oracle/_ref/libchisel_full_ref_o3.so) over {nref} keyframes "
                          f"of the same stream after 5 warm-up keyframes, {rt:.1f} s, 1 thread (the reference is sequential), "
                          f"host has {os.cpu_count()} cores",
                "port": port,
            }

        def deviations(dev, exact):
            ids = {tuple(c) for c in ora.chunk_ids()}
            if ids != {tuple(c) for c in dev.chunk_ids()}:
                return {"ok": False, "why": "chunk sets differ"}
            # Order-free mode.  Stated tolerance: |dsdf| <= 2e-5 m, |dW| / W <= 5e-5 (tests/test_tsdf_chisel.py) — against
            # the EXACT mean of the visits, sum(w_u u) / sum(w_u) in double over the reference's own u and membership.
            # The reference's f32 running mean itself drifts from that mean (every visit re-rounds sdf and W; after N
            # visits by up to ~N * 2^-24 relative), so after thousands of visits per voxel the distance between the two
            # f32 results is dominated by the reference's drift: both distances are reported, per voxel maxima.
            ws = ww = rs = rw = ds_ref = dw_ref = worst_s = worst_w = 0.0
            # ... and against the REFERENCE itself, with the drift its own arithmetic admits: a voxel that has taken n
            # visits holds an f32 running mean that has been re-rounded n times,
            #     |sdf_order_free - sdf_reference| <= 2e-5 m + n * 2^-24 * tau,   |dW| / W <= 5e-5 + n * 2^-24
            # (tau = the truncation distance at max_depth; n is bounded from above by W / w_min, w_min = the weight of a
            # visit at max_depth).  This is the one number an integrator needs: asserted per voxel below.
            z = float(args.max_depth)
            tau = max((0.0019 * z * z - 0.00152 * z + 0.001504) * 6.0, 2.0 * np.sqrt(3.0) * args.resolution)
            w_min = 1.0 / (2.0 * tau)
            for cid in ids:
                a, b = ora.get_chunk(*cid), dev.get_chunk(*cid)
                if not (np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])):
                    return {"ok": False, "why": f"kfid / colour differ in chunk {cid}"}
                known = a[1] > 0
                if not np.array_equal(known, b[1] > 0):
                    return {"ok": False, "why": f"observed voxels differ in chunk {cid}"}
                if exact:
                    if not (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and
                            np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))):
                        return {"ok": False, "why": f"sdf / weight bits differ in chunk {cid}"}
                elif known.any():
                    xs, xw = ora.get_chunk_exact(*cid)
                    ws = max(ws, float(np.abs(b[0][known] - xs[known]).max()))
                    ww = max(ww, float((np.abs(b[1][known] - xw[known]) / xw[known]).max()))
                    rs = max(rs, float(np.abs(a[0][known] - xs[known]).max()))
                    rw = max(rw, float((np.abs(a[1][known] - xw[known]) / xw[known]).max()))
                    ds_ref = max(ds_ref, float(np.abs(a[0][known] - b[0][known]).max()))
                    dw_ref = max(dw_ref, float((np.abs(a[1][known] - b[1][known]) / a[1][known]).max()))
                    n_up = np.ceil(xw[known] / w_min) + 1.0
                    worst_s = max(worst_s, float((np.abs(a[0][known] - b[0][known]) / (2e-5 + n_up * 2.0 ** -24 * tau)).max()))
                    worst_w = max(worst_w, float((np.abs(a[1][known] - b[1][known]) / a[1][known] / (5e-5 + n_up * 2.0 ** -24)).max()))
            if exact:
                return {"ok": True, "chunks": len(ids), "sdf_weight": "bit-identical", "kfid_colour": "identical"}
            return {"ok": ws <= 2e-5 and ww <= 5e-5 and worst_s <= 1.0 and worst_w <= 1.0, "chunks": len(ids),
                    "tolerance": "per voxel with n visits: |dsdf| <= 2e-5 m + n 2^-24 tau and |dW| / W <= 5e-5 + n 2^-24 against the "
                                 f"REFERENCE's f32 map (tau = {tau:.4f} m, the truncation at max_depth; n <= W / w_min), and "
                                 "|dsdf| <= 2e-5 m, |dW| / W <= 5e-5 against the exact (f64) mean of the same visits",
                    "order_free_vs_reference_f32_worst_fraction_of_bound": {"sdf": round(worst_s, 4), "weight": round(worst_w, 4)},
                    "order_free_vs_exact_mean": {"max_abs_sdf_m": ws, "max_rel_weight": ww},
                    "reference_f32_vs_exact_mean": {"max_abs_sdf_m": rs, "max_rel_weight": rw},
                    "order_free_vs_reference_f32": {"max_abs_sdf_m": ds_ref, "max_rel_weight": dw_ref},
                    "kfid_colour": "identical", "observed_voxels": "identical"}

        checks = {("bit_exact_mode" if args.ordered else "order_free_mode"): deviations(tsdf, args.ordered)}
        if t2 is not None:
            checks["order_free_mode" if args.ordered else "bit_exact_mode"] = deviations(t2, not args.ordered)
        result["parity_checked"] = all(c["ok"] for c in checks.values())
        result["parity"] = {"against": f"oracle/tsdf_chisel.c over the same {total_steps * args.batch} keyframes, final map, "
                                       "outside the timed region", **checks}
    if t2 is not None:
        t2.close()


def leg_voxblox_configs3(C):
    # ------------------------------------------------- configs[3]: voxblox 2 cm, a stream of distinct key frames (every N)
    # (main's locals this leg reads)
    TsdfVoxblox = getattr(C, 'TsdfVoxblox', None)
    args = getattr(C, 'args', None)
    b = getattr(C, 'b', None)
    barrier = getattr(C, 'barrier', None)
    f = getattr(C, 'f', None)
    grp = getattr(C, 'grp', None)
    j0 = getattr(C, 'j0', None)
    k = getattr(C, 'k', None)
    leg = getattr(C, 'leg', None)
    make_stream_keyframes = getattr(C, 'make_stream_keyframes', None)
    multi = getattr(C, 'multi', None)
    oracle_lib = getattr(C, 'oracle_lib', None)
    probe = getattr(C, 'probe', None)
    rank = getattr(C, 'rank', None)
    result = getattr(C, 'result', None)
    rounds = getattr(C, 'rounds', None)
    rr = getattr(C, 'rr', None)
    t0 = getattr(C, 't0', None)
    vbx = getattr(C, 'vbx', None)
    world = getattr(C, 'world', None)
    # 25 key frames per step, every step the NEXT 25 of the office loop (depths to 8 m; rays beyond the wrapper's 5 m limit
    # become clearing rays): 2 warm-up + 4 timed steps = 150 distinct key frames.
    if not vbx and not args.no_voxblox_leg:
        vk = make_stream_keyframes(150, first=400, max_depth=8.0, seed=0, threads=min(32, os.cpu_count() or 8))
        for k in vk:
            k["rgba"] = np.concatenate([k["rgb"], np.full((k["rgb"].shape[0], 1), 255, np.uint8)], axis=1)
        vsteps = []
        for j0 in range(0, 150, 25):
            grp = vk[j0:j0 + 25]
            vsteps.append((torch.from_numpy(np.concatenate([k["xyz"] for k in grp])).cuda(),
                           torch.from_numpy(np.concatenate([k["rgba"] for k in grp])).cuda(),
                           np.cumsum([0] + [k["xyz"].shape[0] for k in grp]).astype(np.int32),
                           torch.from_numpy(np.stack([k["Twc"] for k in grp])).cuda()))
        vb = TsdfVoxblox(0.02, max_blocks=65536, shard_rank=rank, shard_count=world)
        for b in vsteps[:2]:
            vb.integrate_batch_dev(*b)
        barrier()
        t0 = time.perf_counter()
        vv = vp = 0
        for b in vsteps[2:]:
            vb.integrate_batch_dev(*b)
            stv = vb.last_stats()
            vv += stv["visits"]
            vp += stv["points"]
        barrier()
        vel = time.perf_counter() - t0
        if multi:
            tt = torch.tensor([vel], dtype=torch.float64, device="cuda")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            vel = float(tt.item())
            tv = torch.tensor([vv], dtype=torch.int64, device="cuda")
            dist.all_reduce(tv, op=dist.ReduceOp.SUM)
            vv_total = int(tv.item())
        else:
            vv_total = vv
        if rank == 0:
            ach = (24.0 * vv + 16.0 * vp) / vel / 1e9
            leg = {
                "metric": "Mvoxels/sec TSDF integrate (voxblox simple 2 cm, office stream, depths to 8 m, max ray 5 m)",
                "value": round(vv_total / vel / 1e6, 2), "unit": "Mvoxels/s", "n_gpus": world, "keyframes_per_step": 25,
                "workload": "configs[3] stand-in, STREAMING: 4 timed steps of 25 DISTINCT key frames each (key frames 450-549 of "
                            "the office loop of tests/synth_scene.py after 2 warm-up steps), Voxblox simple TSDF 2 cm",
                "ms_per_step": round(vel / 4 * 1e3, 3), "visits_per_step": int(vv_total // 4),
                "roofline": {"bound": "hbm", "achieved": round(ach, 2), "peak": 8000.0, "unit": "GB/s",
                             "frac": round(ach / 8000.0, 5), "traffic": None,
                             "note": "24 B per visit + 16 B per point over the wall time of the call (this rank's share)"},
            }
            pmc_v = next((q for q in (os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", f"{rr}_pmc_traffic_voxblox.json")
                                      for rr in ("r06", "r04")) if os.path.exists(q)), "")
            if world == 1 and pmc_v:
                with open(pmc_v) as f:
                    leg["roofline"]["traffic"] = json.load(f)["traffic"]
                leg["roofline"]["traffic_source"] = f"profiles/{os.path.basename(pmc_v)} (FETCH_SIZE x2 + WRITE_SIZE per call)"
            # the reference's own SimpleTsdfIntegrator on the host cores (oracle/_ref/libvoxblox_ref_o3.so: tsdf_integrator.cc
            # compiled unmodified, -O3 -march=x86-64-v3), integrator_threads = 1 and = hardware_concurrency (its default)
            vref = os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracle", "_ref", "libvoxblox_ref_o3.so")
            if world == 1 and not args.no_cpu_baseline and os.path.exists(vref):
                import ctypes as _ct
                from tests import oracle_lib
                _o = oracle_lib.load()
                _o.lib.oracle_voxblox_pose_quat.argtypes = [_ct.c_void_p, _ct.c_void_p]
                _r = _ct.CDLL(vref)
                _r.ref_voxblox_create_threads.restype = _ct.c_void_p
                _r.ref_voxblox_create_threads.argtypes = [_ct.c_float] * 5 + [_ct.c_int, _ct.c_char_p, _ct.c_int]
                _r.ref_voxblox_integrate.argtypes = [_ct.c_void_p] * 5 + [_ct.c_int]
                _r.ref_voxblox_destroy.argtypes = [_ct.c_void_p]
                sample = vk[50:58]                      # the first 8 key frames of the timed steps
                probe = _o.voxblox(0.02)
                rvis = 0
                for k in sample:
                    probe.integrate(k["xyz"], k["rgba"], k["Twc"])
                    rvis += probe.last_visits()         # (the reference exposes no visit counter: the port's count)
                del probe
                base = {}
                for name, nthreads in (("1", 1), ("hardware_concurrency", 0)):
                    hh = _ct.c_void_p(_r.ref_voxblox_create_threads(0.02, 0.1, 10000.0, 0.1, 5.0, 0, b"simple", nthreads))
                    t0 = time.perf_counter()
                    for k in sample:
                        q = np.zeros(4, np.float32)
                        Twc_ = np.ascontiguousarray(k["Twc"], np.float32)
                        _o.lib.oracle_voxblox_pose_quat(Twc_.ctypes.data, q.ctypes.data)
                        tpos = np.ascontiguousarray(Twc_[:, 3])
                        _r.ref_voxblox_integrate(hh, q.ctypes.data, tpos.ctypes.data, k["xyz"].ctypes.data, k["rgba"].ctypes.data,
                                                 k["xyz"].shape[0])
                    base[name] = time.perf_counter() - t0
                    _r.ref_voxblox_destroy(hh)
                leg["cpu_baseline"] = {
                    "value": round(rvis / base["1"] / 1e6, 3), "unit": "Mvoxels/s", "cores": 1, "kind": "reference",
                    "all_cores": {"value": round(rvis / base["hardware_concurrency"] / 1e6, 3), "unit": "Mvoxels/s",
                                  "cores": os.cpu_count(), "integrator_threads": "hardware_concurrency (voxblox's default)"},
                    "sample": f"voxblox::SimpleTsdfIntegrator::integratePointCloud of the reference's own tsdf_integrator.cc (g++ -O3 "
                              f"-march=x86-64-v3, oracle/_ref/libvoxblox_ref_o3.so) over 8 key frames of the timed stream into a "
                              f"fresh 2 cm layer, {base['1']:.1f} s at integrator_threads = 1, {base['hardware_concurrency']:.1f} s at "
                              f"hardware_concurrency; host has {os.cpu_count()} cores"}
                # ---- the "fast" method (PLVS's YAML default): the device's one-thread schedule against the reference's
                # own FastTsdfIntegrator on the same 8 key frames, one scan per call as PLVS issues them
                try:
                    vf = TsdfVoxblox(0.02, max_blocks=65536)
                    hh = _ct.c_void_p(_r.ref_voxblox_create_threads(0.02, 0.1, 10000.0, 0.1, 5.0, 0, b"fast", 1))
                    t_ref = t_hip = 0.0
                    fvis = rounds = 0
                    for k in sample:
                        q = np.zeros(4, np.float32)
                        Twc_ = np.ascontiguousarray(k["Twc"], np.float32)
                        _o.lib.oracle_voxblox_pose_quat(Twc_.ctypes.data, q.ctypes.data)
                        tpos = np.ascontiguousarray(Twc_[:, 3])
                        t0 = time.perf_counter()
                        _r.ref_voxblox_integrate(hh, q.ctypes.data, tpos.ctypes.data, k["xyz"].ctypes.data, k["rgba"].ctypes.data,
                                                 k["xyz"].shape[0])
                        t_ref += time.perf_counter() - t0
                        t0 = time.perf_counter()
                        vf.integrate_fast(k["xyz"], k["rgba"], k["Twc"])
                        t_hip += time.perf_counter() - t0
                        fvis += vf.last_stats()["visits"]
                        rounds = max(rounds, vf.fast_rounds())
                    _r.ref_voxblox_destroy(hh)
                    # bit identity: against the reference built WITHOUT floating-point contraction (libvoxblox_ref.so, the build
                    # the oracle is pinned by; the -O3 -march build above fuses multiply-adds: DESIGN §3)
                    _p = _ct.CDLL(vref.replace("libvoxblox_ref_o3.so", "libvoxblox_ref.so"))
                    _p.ref_voxblox_create.restype = _ct.c_void_p
                    _p.ref_voxblox_create.argtypes = [_ct.c_float] * 5 + [_ct.c_int, _ct.c_char_p]
                    _p.ref_voxblox_integrate.argtypes = [_ct.c_void_p] * 5 + [_ct.c_int]
                    _p.ref_voxblox_num_blocks.argtypes = [_ct.c_void_p]
                    _p.ref_voxblox_block_ids.argtypes = [_ct.c_void_p, _ct.c_void_p]
                    _p.ref_voxblox_get_block.argtypes = [_ct.c_void_p] + [_ct.c_int] * 3 + [_ct.c_void_p] * 3
                    _p.ref_voxblox_destroy.argtypes = [_ct.c_void_p]
                    hh = _ct.c_void_p(_p.ref_voxblox_create(0.02, 0.1, 10000.0, 0.1, 5.0, 0, b"fast"))
                    for k in sample:
                        q = np.zeros(4, np.float32)
                        Twc_ = np.ascontiguousarray(k["Twc"], np.float32)
                        _o.lib.oracle_voxblox_pose_quat(Twc_.ctypes.data, q.ctypes.data)
                        tpos = np.ascontiguousarray(Twc_[:, 3])
                        _p.ref_voxblox_integrate(hh, q.ctypes.data, tpos.ctypes.data, k["xyz"].ctypes.data, k["rgba"].ctypes.data,
                                                 k["xyz"].shape[0])
                    nbk = _p.ref_voxblox_num_blocks(hh)
                    bids = np.zeros((max(nbk, 1), 3), np.int32)
                    _p.ref_voxblox_block_ids(hh, bids.ctypes.data)
                    same = nbk == vf.num_chunks()
                    for bid in bids[:nbk]:
                        d_, w_, c_ = np.zeros(4096, np.float32), np.zeros(4096, np.float32), np.zeros(4096, np.uint32)
                        _p.ref_voxblox_get_block(hh, int(bid[0]), int(bid[1]), int(bid[2]), d_.ctypes.data, w_.ctypes.data, c_.ctypes.data)
                        g_ = vf.get_chunk(*bid)
                        same = same and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip((d_, w_, c_), g_))
                    _p.ref_voxblox_destroy(hh)
                    vf.close()
                    leg["fast_method"] = {
                        "what": "FastTsdfIntegrator (PointCloudMapping.voxbloxIntegrationMethod: fast), one key frame per call, host "
                                "flavour, 8 key frames into a fresh 2 cm layer: the device's one-thread schedule against the reference's "
                                "own integrator at integrator_threads = 1",
                        "hip_ms_per_keyframe": round(t_hip / len(sample) * 1e3, 3), "reference_cpu_ms_per_keyframe": round(t_ref / len(sample) * 1e3, 2),
                        "voxel_updates": int(fvis), "simple_voxel_updates": int(rvis), "rounds_max": int(rounds),
                        "bit_identical_to_the_reference_layer": bool(same), "blocks": int(nbk)}
                except Exception as e:   # (a reported leg, never the headline)
                    leg["fast_method"] = {"error": repr(e)}
            result["voxblox_configs3"] = leg
        vb.close()


def leg_frontend(C):
    # ------------------------------------------------- front end (N = 1 only)
    # (main's locals this leg reads)
    TsdfChisel = getattr(C, 'TsdfChisel', None)
    _ct = getattr(C, '_ct', None)
    _lib = getattr(C, '_lib', None)
    args = getattr(C, 'args', None)
    e = getattr(C, 'e', None)
    f = getattr(C, 'f', None)
    k = getattr(C, 'k', None)
    leg = getattr(C, 'leg', None)
    name = getattr(C, 'name', None)
    names = getattr(C, 'names', None)
    ora = getattr(C, 'ora', None)
    oracle_lib = getattr(C, 'oracle_lib', None)
    pinned = getattr(C, 'pinned', None)
    q = getattr(C, 'q', None)
    rank = getattr(C, 'rank', None)
    result = getattr(C, 'result', None)
    same = getattr(C, 'same', None)
    st = getattr(C, 'st', None)
    t = getattr(C, 't', None)
    t0 = getattr(C, 't0', None)
    ts = getattr(C, 'ts', None)
    ts_ = getattr(C, 'ts_', None)
    v = getattr(C, 'v', None)
    w_ = getattr(C, 'w_', None)
    world = getattr(C, 'world', None)
    if rank == 0 and world == 1 and not args.no_frontend:
        from plvs_amd.matcher import knn2_raw
        rng = np.random.default_rng(1)
        q = torch.from_numpy(rng.integers(0, 256, (2000, 32), dtype=np.uint8)).cuda()
        t = torch.from_numpy(rng.integers(0, 256, (2000, 32), dtype=np.uint8)).cuda()
        fe = {}
        for name, rule in (("orb_bf_2000x2000", _lib.TIE_LOWEST_INDEX), ("lbd_mih_2000x2000", _lib.TIE_MIH)):
            for _ in range(5):
                knn2_raw(q, t, None, rule)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                knn2_raw(q, t, None, rule)
            e1.record()
            torch.cuda.synchronize()
            fe[name + "_us"] = round(e0.elapsed_time(e1) / 50 * 1e3, 2)
        # ORB(2000) extraction on a 640x480 frame resident in HBM (configs[1] front end)
        from plvs_amd.orb import ORBextractor
        from tests.pgm import golden_frame as golden
        frames = [torch.from_numpy(golden(n)).cuda() for n in ("aloe_640x480.pgm", "aloe_640x480_shift.pgm",
                                                                "cones_640x480.pgm")]
        ext = ORBextractor(2000, 1.2, 8, 20, 7)
        for i in range(6):
            ext(frames[i % 3])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nrep, nk = 30, 0
        stage = {}
        for i in range(nrep):
            mono, kps, desc = ext(frames[i % 3])
            nk += len(kps)
            for k, v in ext.stage_ms().items():
                stage[k] = stage.get(k, 0.0) + v
        orb_ms = (time.perf_counter() - t0) / nrep * 1e3
        ext.close()
        # EDLines + LBD (100 lines, 3 levels) on the same frames
        from plvs_amd.lines import LineExtractor
        lext = LineExtractor(100)
        for i in range(4):
            lext(frames[i % 3])
        t0 = time.perf_counter()
        lstage, nlines = {}, 0
        for i in range(nrep):
            kl, ld = lext(frames[i % 3])
            nlines += len(kl)
            for k, v in lext.stage_ms().items():
                lstage[k] = lstage.get(k, 0.0) + v
        lines_ms = (time.perf_counter() - t0) / nrep * 1e3
        # the reference extracts points and lines on two host threads (src/Frame.cc:503-508)
        from plvs_amd.frame import extract_frame
        ext2 = ORBextractor(2000, 1.2, 8, 20, 7)
        for i in range(8):
            extract_frame(ext2, lext, frames[i % 3])
        t0 = time.perf_counter()
        for i in range(2 * nrep):
            extract_frame(ext2, lext, frames[i % 3])
        both_ms = (time.perf_counter() - t0) / (2 * nrep) * 1e3
        ext2.close()
        lext.close()
        # LBD k-NN at the real size (100 x 100 lines)
        q100 = torch.from_numpy(rng.integers(0, 256, (100, 32), dtype=np.uint8)).cuda()
        for _ in range(5):
            knn2_raw(q100, q100, None, _lib.TIE_MIH)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            knn2_raw(q100, q100, None, _lib.TIE_MIH)
        e1.record()
        torch.cuda.synchronize()
        fe["lbd_mih_100x100_us"] = round(e0.elapsed_time(e1) / 50 * 1e3, 2)
        front_ms = both_ms + (fe["orb_bf_2000x2000_us"] + fe["lbd_mih_100x100_us"]) * 1e-3
        result["frontend"] = {
            "metric": "frames/sec front-end (ORB 2000 + EDLines/LBD 100x3 + Hamming match), 640x480, 1 GPU",
            "frames_per_s": round(1e3 / front_ms, 1), "ms_per_frame": round(front_ms, 3),
            "orb_extract_ms": round(orb_ms, 3), "lines_extract_ms": round(lines_ms, 3),
            "orb_and_lines_two_threads_ms": round(both_ms, 3),
            "orb_keypoints_per_frame": nk // nrep, "lines_per_frame": nlines // nrep,
            "orb_stage_ms": {k: round(v / nrep, 3) for k, v in stage.items()},
            "lines_stage_ms": {k: round(v / nrep, 3) for k, v in lstage.items()},
            "hamming_knn2": fe,
            "note": "match = one brute-force 2000x2000 ORB k-NN + one 100x100 LBD k-NN per frame",
        }
        # ---- every search function at the working sizes (host flavour: what PLVS's Tracking would call), beside
        # the CPU restatement of the same call.  2000 keypoints x 1500 map points, 300 x 250 lines.
        try:
            from plvs_amd.linematcher import LineMatcher, line_frame_view
            from plvs_amd.orbmatcher import ORBmatcher
            from tests import oracle_lib
            from tests import test_line_proj_search as tlp
            from tests import test_line_search as tls
            from tests import test_orb_search as tos
            ora = oracle_lib.load()

            def per_call_us(fn, reps=30):   # median: one allocator hiccup of the process would otherwise decide a 50 us figure
                fn()
                fn()
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    fn()
                    ts.append(time.perf_counter() - t0)
                return round(float(np.median(ts)) * 1e6, 1)

            mt = {}
            F, M, occ = tos.make_case(1, n=2000, m=1500)
            om = ORBmatcher(0.8, True)
            mt["orb_search_by_projection_mappoints"] = {
                "hip_us": per_call_us(lambda: om.SearchByProjection(F, M, 1.0, False, 40.0, occupied=occ)),
                "cpu_us": per_call_us(lambda: tos.oracle_search(ora.lib, F, M, 1.0, False, 40.0, 0.8, occ), 10)}
            F2, ang, mx, my, mbf, L, occ2 = tos.make_ff_case(1, n=2000)
            om2 = ORBmatcher(0.9, True)
            mt["orb_search_by_projection_lastframe"] = {
                "hip_us": per_call_us(lambda: om2.SearchByProjectionLastFrame(F2, ang, mx, my, mbf, L, 15.0, False, False,
                                                                              occupied=occ2)),
                "cpu_us": per_call_us(lambda: tos.oracle_search_ff(ora.lib, F2, ang, mx, my, mbf, L, 15.0, 0, 0, 1, occ2), 10)}
            KV, kd, kv, ka, FV, fd, fa = tos.make_bow_case(1, nk=2000, nf=2000)
            om3 = ORBmatcher(0.7, True)
            mt["orb_search_by_bow"] = {
                "hip_us": per_call_us(lambda: om3.SearchByBoW(KV, kd, kv, ka, FV, fd, fa)),
                "cpu_us": per_call_us(lambda: tos.oracle_search_bow(ora.lib, KV, kd, kv, ka, FV, fd, fa, 0.7, 1), 10)}
            lc = tls.make_case(1, n_last=250, n_cur=300)
            lm = LineMatcher(0.8, True)
            mt["lines_search_by_knn_keyframe"] = {
                "hip_us": per_call_us(lambda: lm.SearchByKnn(lc[0], lc[1], lc[2], lc[3], lc[4])),
                "cpu_us": per_call_us(lambda: tls.run(tls.oracle_fn(ora), lc, 0.8, True), 10)}
            pc = tlp.make_case(1, n_cur=300, n_last=250)
            view = line_frame_view(pc["kl"], pc["desc"], tlp.SCALE, tlp.INV_SIGMA2, tlp.MAX_DIAG)
            mt["lines_search_by_projection_lastframe"] = {
                "hip_us": per_call_us(lambda: lm.SearchByProjectionLastFrame(view, pc["valid"], pc["proj"], pc["octave"],
                                                                              pc["angle"], pc["ldesc"],
                                                                              occupied=pc["occupied"], has_obs=pc["has_obs"])),
                "cpu_us": per_call_us(lambda: tlp.oracle_ff(ora, pc, False, 0, 0.8, True), 10)}
            mt["lines_search_by_projection_maplines"] = {
                "hip_us": per_call_us(lambda: lm.SearchByProjection(view, pc["valid"], pc["proj_map"], pc["octave"], pc["ldesc"],
                                                                    occupied=pc["occupied"], has_obs=pc["has_obs"])),
                "cpu_us": per_call_us(lambda: tlp.oracle_map(ora, pc, False, 0.8), 10)}
            # ---- the tracking step on REAL extractor output: frame upload, ORB + lines of aloe_shift, and
            # ORBmatcher::SearchByProjection(CurrentFrame, LastFrame) of its keypoints against the previous frame's
            # (aloe: the same scene cropped 3 px / 2 px further left / up, so a last-frame keypoint at (x, y) projects
            # to (x - 3, y - 2); every last-frame keypoint stands for a map point 2 m away)
            from plvs_amd.orbmatcher import FrameView, LastFrameView
            ext3, lext3 = ORBextractor(2000, 1.2, 8, 20, 7), LineExtractor(100)
            scale = np.asarray(ext3.GetScaleFactors(), np.float32)
            pinned = [torch.from_numpy(golden(n)).pin_memory() for n in ("aloe_640x480.pgm", "aloe_640x480_shift.pgm")]
            _, k0, d0, l0, ld0 = extract_frame(ext3, lext3, pinned[0].cuda())
            # last frame's lines as map lines projected into the current frame (same 3 px / 2 px shift, 2 m away)
            lproj = np.stack([l0["startPointX"] - 3.0, l0["startPointY"] - 2.0, l0["endPointX"] - 3.0, l0["endPointY"] - 2.0,
                              np.full(len(l0), 0.5), np.full(len(l0), 0.5)], axis=1).astype(np.float32)
            lvalid = np.ones(len(l0), np.uint8)
            lm4 = LineMatcher(0.8, True)
            last = LastFrameView(valid=np.ones(len(k0), np.uint8), u=k0["x"] - 3.0, v=k0["y"] - 2.0,
                                 invz=np.full(len(k0), 0.5, np.float32), octave=k0["octave"], angle=k0["angle"], desc=d0)
            om4 = ORBmatcher(0.9, True)

            no_uright = np.full(4096, -1.0, np.float32)

            def match_points(k1, d1):      # runs as soon as the points are out, beside the line thread
                cur = FrameView(k1["x"], k1["y"], k1["octave"], no_uright[:len(k1)], d1, 0.0, 0.0,
                                64.0 / 640.0, 48.0 / 480.0, scale)
                return om4.SearchByProjectionLastFrame(cur, k1["angle"], 640.0, 480.0, 40.0, last, 15.0)

            def track_once():
                img = pinned[1].cuda(non_blocking=True)
                _, k1, d1, l1, ld1, hooked = extract_frame(ext3, lext3, img, after_points=match_points)
                lview = line_frame_view(l1, ld1, tlp.SCALE, tlp.INV_SIGMA2, tlp.MAX_DIAG)
                nl_, _ = lm4.SearchByProjectionLastFrame(lview, lvalid, lproj, l0["octave"], l0["angle"], ld0)
                track_once.line_matches = nl_
                cur = FrameView(k1["x"], k1["y"], k1["octave"], no_uright[:len(k1)], d1, 0.0, 0.0,
                                64.0 / 640.0, 48.0 / 480.0, scale)
                return hooked, cur, k1

            (nm, _), cur, k1 = track_once()
            real_us = per_call_us(lambda: track_once(), 30)
            match_us = per_call_us(lambda: om4.SearchByProjectionLastFrame(cur, k1["angle"], 640.0, 480.0, 40.0, last, 15.0), 30)
            cpu_match_us = per_call_us(lambda: tos.oracle_search_ff(ora.lib, cur, np.ascontiguousarray(k1["angle"], np.float32),
                                                                   640.0, 480.0, 40.0, last, 15.0, 0, 0, 1,
                                                                   np.zeros(len(k1), np.uint8)), 10)
            ext3.close()
            lext3.close()
            result["frontend"]["real_pair_tracking_step"] = {
                "what": "pinned host frame -> HBM, ORB 2000 || EDLines/LBD 100x3, ORBmatcher and LineMatcher "
                        "SearchByProjection(CurrentFrame, LastFrame) of aloe_shift against aloe's keypoints and lines "
                        "(host flavours); the ORB search runs in plvs_hip_frame_extract_dev_hook's after-points hook, "
                        "beside the line thread",
                "ms_per_frame": round(real_us * 1e-3, 3), "search_by_projection_us": match_us,
                "search_by_projection_cpu_us": cpu_match_us, "matches": int(nm),
                "line_matches": int(getattr(track_once, "line_matches", -1)),
                "keypoints": [int(len(k0)), int(len(k1))]}
            # the front end's headline: the real tracking step (the extraction + synthetic k-NN figure stays beside it)
            fe_ = result["frontend"]
            fe_["extraction_plus_knn_ms_per_frame"] = fe_["ms_per_frame"]
            fe_["ms_per_frame"] = round(real_us * 1e-3, 3)
            fe_["frames_per_s"] = round(1e6 / real_us, 1)
            fe_["metric"] = ("frames/sec front-end: frame upload + ORB 2000 || EDLines/LBD 100x3 + ORB and line "
                             "SearchByProjection against the previous frame, 640x480 real pair, 1 GPU")
            mt["note"] = ("host flavours (inputs in host memory, one staged copy in and out per call) on synthetic frames of "
                          "the working size; cpu_us = oracle/*.c (the reference's loop, one core), both through ctypes")
            result["frontend"]["search_functions"] = mt
            # ---- CPU baseline of the extraction: the reference's two threads (src/Frame.cc:503-508)
            import threading
            host_frames = [f.cpu().numpy() for f in frames]
            o_orb, o_lines = ora.orb(2000, 1.2, 8, 20, 7), ora.lines()
            ncpu = 100
            for i in range(10):      # warm-up (>= 100 frames after 10 warm-ups)
                o_orb.extract(host_frames[i % 3])
                o_lines.extract(host_frames[i % 3])
            t0 = time.perf_counter()
            for i in range(ncpu):
                img = host_frames[i % 3]
                th_ = [threading.Thread(target=o_orb.extract, args=(img,)), threading.Thread(target=o_lines.extract, args=(img,))]
                for t_ in th_:
                    t_.start()
                for t_ in th_:
                    t_.join()
            cpu_ms = (time.perf_counter() - t0) / ncpu * 1e3
            result["frontend"]["cpu_baseline"] = {
                "value": round(1e3 / cpu_ms, 2), "unit": "frames/s", "ms_per_frame": round(cpu_ms, 2), "cores": 2,
                "kind": "port", "sample": f"oracle/orb.cpp || oracle/lines.cpp on two threads, {ncpu} frames after 10 warm-up "
                                          f"frames (extraction only), host has {os.cpu_count()} cores"}
            # the reference's own extractors where they have been built (oracle/_ref/libfrontend_ref_o3.so: src/ORBextractor.cc,
            # src/LineExtractor.cc, binary_descriptor_custom.cpp compiled unmodified, -O3 -march=x86-64-v3, against the OpenCV
            # stand-in whose image primitives are this repository's restatements): the same two threads
            fref = os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracle", "_ref", "libfrontend_ref_o3.so")
            if os.path.exists(fref):
                import ctypes as _ct
                from tests.oracle_lib import OracleLines
                from tests.test_oracle_pinned_frontend import _RefNames, _RefOrb
                names = _RefNames(_ct.CDLL(fref))
                r_orb, r_lines = _RefOrb(names, 2000), OracleLines(names)
                for i in range(10):
                    r_orb.extract(host_frames[i % 3])
                    r_lines.extract(host_frames[i % 3])
                t0 = time.perf_counter()
                for i in range(ncpu):
                    img = host_frames[i % 3]
                    th_ = [threading.Thread(target=r_orb.extract, args=(img,)), threading.Thread(target=r_lines.extract, args=(img,))]
                    for t_ in th_:
                        t_.start()
                    for t_ in th_:
                        t_.join()
                ref_ms = (time.perf_counter() - t0) / ncpu * 1e3
                result["frontend"]["cpu_baseline"] = {
                    "value": round(1e3 / ref_ms, 2), "unit": "frames/s", "ms_per_frame": round(ref_ms, 2), "cores": 2,
                    "kind": "reference", "port_ms_per_frame": round(cpu_ms, 2),
                    "sample": f"PLVS2::ORBextractor::operator() || PLVS2::LineExtractor::operator() of the reference's own sources "
                              f"(oracle/_ref/libfrontend_ref_o3.so, g++ -O3 -march=x86-64-v3; OpenCV's image primitives are the "
                              f"repository's restatements) on two threads as src/Frame.cc:503-508 runs them, {ncpu} frames after 10 "
                              f"warm-up frames (extraction only), host has {os.cpu_count()} cores"}
        except Exception as e:      # the timing harness must not take the benchmark line down
            result["frontend"]["search_functions"] = {"error": repr(e)}
        # configs[4] (KITTI stereo): dense disparity by semi-global matching on a 1240x376 pair resident in HBM
        from plvs_amd.sgm import StereoSGM
        sl = torch.from_numpy(np.ascontiguousarray(golden("urban1_1241x376.pgm")[:, :1240])).cuda()
        sr = torch.from_numpy(np.ascontiguousarray(golden("urban1_right_1241x376.pgm")[:, :1240])).cuda()
        sgm = StereoSGM(1240, 376)
        sd = torch.zeros((376, 1240), dtype=torch.uint8, device="cuda")
        for _ in range(3):
            sgm.execute_dev(sl, sr, sd)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            sgm.execute_dev(sl, sr, sd)
        e1.record()
        torch.cuda.synchronize()
        result["frontend"]["dense_stereo_sgm"] = {
            "ms_per_pair": round(e0.elapsed_time(e1) / 20, 3), "size": "1240x376, 64 disparities, 8 paths",
            "valid_fraction": round(float((sd > 0).float().mean()), 3)}

        # the line extractor with Line.LSD.on: 1 (row L9): plvs_hip_lsd_extract, 100 lines, three octaves, the options Tracking
        # passes; beside it the reference's own sources (oracle/_ref/liblsd_ref.so) on one core where they have been built
        try:
            from plvs_amd.lines import LineExtractor as _LX, LSDOptions as _LO

            class _Lsd(_LX):
                skUseLsdExtractor = True
            lsd_img = np.ascontiguousarray(golden("aloe_640x480.pgm"))
            lsd_opts = dict(refine=1, scale=float(np.float32(1.2)), sigma_scale=0.6, quant=2.0, ang_th=22.5, log_eps=1.0,
                            density_th=0.6, n_bins=1024)
            lx_ = _Lsd(100, _LO(numOctaves=3, min_length=0.025, **lsd_opts))
            lx_(lsd_img)
            ts_ = []
            for _ in range(10):
                t0 = time.perf_counter()
                lkl, ldesc = lx_(lsd_img)
                ts_.append((time.perf_counter() - t0) * 1e3)
            leg = {"what": "LineExtractor::operator() with skUseLsdExtractor on a 640x480 frame, host image in, KeyLines + LBD out",
                   "ms_per_frame": round(sorted(ts_)[len(ts_) // 2], 2), "ms_min": round(min(ts_), 2), "lines": int(len(lkl)),
                   "stage_ms": {k: round(v, 2) for k, v in lx_.stage_ms().items()}}
            lx_.close()
            lref = os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracle", "_ref", "liblsd_ref.so")
            if os.path.exists(lref):
                from tests.test_lsd import RefBackend as _LsdRef
                rb_ = _LsdRef()
                t0 = time.perf_counter()
                for _ in range(3):
                    rkl, rdesc = rb_.extract(lsd_img, 100, 3, lsd_opts, 0.025)
                ref_ms = (time.perf_counter() - t0) / 3 * 1e3
                leg["cpu_baseline"] = {"ms_per_frame": round(ref_ms, 1), "cores": 1, "kind": "reference",
                                       "sample": "the reference's lsd_custom.cpp / LSDDetector_custom.cpp / LineExtractor.cc "
                                                 "(oracle/_ref/liblsd_ref.so, g++ -O2; image primitives are the stand-in's), 3 calls"}
                leg["parity_ok"] = bool(len(rkl) == len(lkl) and rkl.tobytes() == lkl.tobytes() and rdesc.tobytes() == ldesc.tobytes())
            result["frontend"]["lsd_extract"] = leg
        except Exception as e:
            result["frontend"]["lsd_extract"] = {"error": repr(e)}

        # dense disparity by libelas: the stages on the device — the candidate loop of computeSupportMatches and the two
        # methods the reference's GPU build overrides — on the arguments the reference's own pipeline produces for that pair
        # (oracle/_ref/libelas_ref.so: test infrastructure, the CPU baseline of this leg)
        try:
            import ctypes as _ct
            from tests import elas_ref
            if not elas_ref.available():
                raise RuntimeError("oracle/_ref/libelas_ref.so is not built here")
            from plvs_amd.elas import ElasGPU
            el, er = golden("urban1_1241x376.pgm"), golden("urban1_right_1241x376.pgm")
            _rl = _ct.CDLL(elas_ref.REF)
            _rl.ref_elas_stage_seconds.argtypes = [_ct.c_void_p] * 2 + [_ct.c_int] * 5 + [_ct.c_void_p]
            leg = {}
            for sub in (False, True):
                dcalls, mcalls, ref_out = elas_ref.capture(el, er, subsampling=sub, plvs=True)
                eg = ElasGPU(ElasGPU.Parameters(subsampling=sub))
                d0 = dcalls[0]       # (the descriptor pair of the run: the same images go to computeSupportMatches)

                def hip_pair():
                    eg.setImages(el, er)         # the descriptor images on the device, staged for the stages below
                    eg.supportCandidates(None, None, d0["width"], d0["height"])
                    Ds = [eg.computeDisparity(a["support"], a["tri"], a["grid"], a["grid_dims"], None, None, a["right_image"],
                                              a["width"], a["height"]) for a in dcalls]     # the pair is staged by supportCandidates
                    D1, D2 = eg.leftRightConsistencyCheck(Ds[0], Ds[1], d0["width"], d0["height"])
                    D1 = eg.removeSmallSegments(D1, d0["width"], d0["height"])               # PLVS: postprocess_only_left
                    D1 = eg.gapInterpolation(D1, d0["width"], d0["height"])
                    return eg.adaptiveMean(D1, d0["width"], d0["height"]), D2
                got = hip_pair()
                same = all(np.array_equal(g.reshape(-1).view(np.uint32), w.reshape(-1).view(np.uint32)) for g, w in zip(got, ref_out))
                t0 = time.perf_counter()
                for _ in range(10):
                    hip_pair()
                hip_ms = (time.perf_counter() - t0) / 10 * 1e3
                # the reference's compiled pipeline, seconds per stage (oracle/ref/elas_ref_wrap.cpp), best of three runs
                best = None
                for _ in range(3):
                    st = np.zeros(11)
                    _rl.ref_elas_stage_seconds(el.ctypes.data, er.ctypes.data, el.shape[1], el.shape[0], el.shape[1], 1, int(sub),
                                               st.ctypes.data)
                    best = st if best is None or st[10] < best[10] else best
                _rl.ref_elas_descriptor.argtypes = [_ct.c_void_p] + [_ct.c_int] * 4 + [_ct.c_void_p]
                dbuf = np.zeros(16 * el.size, np.uint8)
                t0 = time.perf_counter()
                for im in (el, er):
                    _rl.ref_elas_descriptor(im.ctypes.data, im.shape[1], im.shape[0], im.shape[1], int(sub), dbuf.ctypes.data)
                desc_s = time.perf_counter() - t0
                moved = best[0] + best[4] + best[5] + best[6] + best[7] + best[9] + desc_s
                leg["subsampling" if sub else "full_resolution"] = {
                    "hip_ms_per_pair": round(hip_ms, 3), "cpu_ms_per_pair": round(moved * 1e3, 3),
                    "cpu_descriptors_ms": round(desc_s * 1e3, 3),
                    "cpu_support_matches_ms": round(best[0] * 1e3, 3), "cpu_compute_disparity_ms": round(best[4] * 1e3, 3),
                    "cpu_lr_check_speckles_gaps_ms": round((best[5] + best[6] + best[7]) * 1e3, 3),
                    "cpu_adaptive_mean_ms": round(best[9] * 1e3, 3), "bit_identical": bool(same),
                    "reference_pipeline_ms": round(best[10] * 1e3, 1),
                    "reference_pipeline_rest_ms": round((best[10] - moved) * 1e3, 1)}
            leg["what"] = ("libelas::Descriptor of both images, the candidate loop of Elas::computeSupportMatches, Elas::computeDisparity (left + right image), "
                           "leftRightConsistencyCheck, removeSmallSegments, gapInterpolation and adaptiveMean (left map, as PLVS sets "
                           "postprocess_only_left) of the 1241x376 pair: what ElasGPU moves to the device and four stages more, each "
                           "through its host-pointer entry point (images uploaded once per pair, the descriptor images never leave HBM, "
                           "triangles and grids per call, every map read back and uploaded again between stages); bit_identical = the final maps against "
                           "the reference pipeline's; cpu = the same stages inside the reference's compiled Elas::process, 1 thread "
                           "(support matches include its host filters); reference_pipeline_rest_ms = what stays on the host: "
                           "support filters, triangulation, planes, grid (the descriptors are timed apart: the pipeline's own timer "
                           "does not separate them)")
            result["frontend"]["dense_stereo_elas"] = leg
        except Exception as e:
            result["frontend"]["dense_stereo_elas"] = {"skipped": repr(e)}

        # ---- configs[4] as the shipped YAML runs it (KITTI00-02.yaml: 1241x376 stereo, libelas, chisel 10 cm), one key frame:
        # ORB 2000 || EDLines/LBD on the left image, the libelas pair with every device stage (the two disparity maps stay in
        # HBM, the post-processing is one call), disparity -> depth -> cloud with normals on the device, one 10 cm integrate
        try:
            from tests import elas_ref
            from plvs_amd import cloudgen
            from plvs_amd.elas import ElasGPU
            if not elas_ref.available():
                raise RuntimeError("oracle/_ref/libelas_ref.so is not built here")
            kl_, kr_ = golden("urban1_1241x376.pgm"), golden("urban1_right_1241x376.pgm")
            kh, kw = kl_.shape
            kfx, kcx, kcy, kbf = 718.856, 607.1928, 185.2157, 386.1448
            ext_k, lext_k = ORBextractor(2000, 1.2, 8, 20, 7), LineExtractor(100)
            d_left = torch.from_numpy(kl_).cuda()
            eg = ElasGPU(ElasGPU.Parameters(subsampling=True))
            kgrid = cloudgen.InitCamGridPoints(kw, kh, 2, kfx, kfx, kcx, kcy)
            kgen = cloudgen.PointCloudGenerator(kw, kh, kgrid, step=2, min_depth=0.5, max_depth=20.0)
            d_bgr = torch.from_numpy(np.repeat(kl_[:, :, None], 3, axis=2)).cuda()
            d_depth = torch.empty((kh, kw), dtype=torch.float32, device="cuda")
            d_xyz = torch.empty((kgen.ngrid, 3), dtype=torch.float32, device="cuda")
            d_rgb = torch.empty((kgen.ngrid, 3), dtype=torch.uint8, device="cuda")
            d_kf = torch.empty(kgen.ngrid, dtype=torch.int32, device="cuda")
            kTwc = torch.from_numpy(np.eye(4, dtype=np.float32)[None, :3]).cuda()
            kmap = TsdfChisel(0.10, max_chunks=16384, order_free=True)
            stage = {}

            def clock(name, fn):
                torch.cuda.synchronize()
                t0_ = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                stage[name] = stage.get(name, 0.0) + (time.perf_counter() - t0_)
                return out

            def elas_pair():
                eg.setImages(kl_, kr_)

                def chain(D1, D2):
                    D1[:], D2[:] = eg.postProcess(kw, kh, postprocess_only_left=True, filter_adaptive_mean=True)
                return elas_ref.run_with(
                    kl_, kr_, lambda a: eg.computeDisparity(a["support"], a["tri"], a["grid"], a["grid_dims"], None, None,
                                                            a["right_image"], kw, kh),
                    lambda D, ww, hh, sub: D, subsampling=True, plvs=True,
                    support_candidates=lambda a: eg.supportCandidates(None, None, kw, kh),
                    post=dict(left_right_check=chain, remove_small_segments=lambda D: None, gap_interpolation=lambda D: None))

            def cloud_and_map():
                eg.depthDev(kbf, 2, d_depth)
                npts = kgen.generate_dev(d_bgr, d_depth, 7, d_xyz, d_rgb=d_rgb, d_kfid=d_kf)
                kmap.integrate_batch_dev(d_xyz, d_rgb, d_kf, np.array([0, npts], np.int32), kTwc)
                return npts

            for _ in range(3):
                extract_frame(ext_k, lext_k, d_left)
                elas_pair()
                cloud_and_map()
            stage.clear()
            nrep_k = 10
            for _ in range(nrep_k):
                clock("orb_and_lines", lambda: extract_frame(ext_k, lext_k, d_left))
                maps = clock("libelas_pair_incl_reference_host_stages", elas_pair)
                npts = clock("depth_cloud_integrate_10cm", cloud_and_map)
            want_maps = elas_ref.reference(kl_, kr_, subsampling=True, plvs=True)
            # CPU beside: the reference pipeline itself, the oracles' extraction on two threads, cloud + integrate by the ports
            t0 = time.perf_counter()
            elas_ref.reference(kl_, kr_, subsampling=True, plvs=True)
            cpu_elas = time.perf_counter() - t0
            o_orb_k, o_lines_k = ora.orb(2000, 1.2, 8, 20, 7), ora.lines()
            t0 = time.perf_counter()
            th_ = [threading.Thread(target=o_orb_k.extract, args=(kl_,)), threading.Thread(target=o_lines_k.extract, args=(kl_,))]
            for t_ in th_:
                t_.start()
            for t_ in th_:
                t_.join()
            cpu_fe = time.perf_counter() - t0
            depth_h = d_depth.cpu().numpy()
            t0 = time.perf_counter()
            rec_k, _ = ora.cloudgen(depth_h, np.repeat(kl_[:, :, None], 3, axis=2), kgrid, 2, 0.5, 20.0, 7)
            o_map = ora.chisel(0.10)
            o_map.integrate(np.stack([rec_k["x"], rec_k["y"], rec_k["z"]], -1), np.stack([rec_k["r"], rec_k["g"], rec_k["b"]], -1),
                            rec_k["kfid"], np.eye(4, dtype=np.float32)[:3])
            cpu_cloud = time.perf_counter() - t0
            result["kitti_shaped"] = {
                "what": "configs[4] as shipped (Examples_old/Stereo/KITTI00-02.yaml: 1241x376 stereo, libelas with subsampling, chisel "
                        "10 cm), one key frame: ORB 2000 || EDLines/LBD 100x3 on the left image; the libelas pair with every device "
                        "stage (descriptors, support candidates, computeDisparity x2 left in HBM, the post-processing chain as one "
                        "call) inside the reference's own Elas::process, whose host stages (support filters, triangulation, planes, "
                        "grid) run on one core; disparity -> depth -> cloud with normals on the device and one order-free integrate",
                "ms_per_keyframe": round(sum(stage.values()) / nrep_k * 1e3, 3),
                "stage_ms": {k: round(v / nrep_k * 1e3, 3) for k, v in stage.items()},
                "points": int(npts), "disparity_maps_bit_identical_to_reference": bool(
                    all(np.array_equal(g.view(np.uint32), w_.view(np.uint32)) for g, w_ in zip(maps, want_maps))),
                "cpu_ms": {"orb_and_lines_two_threads_port": round(cpu_fe * 1e3, 2), "libelas_reference_pipeline": round(cpu_elas * 1e3, 2),
                           "cloud_and_integrate_port": round(cpu_cloud * 1e3, 2), "cores": 2}}
            kmap.close()
            eg.close()
            ext_k.close()
            lext_k.close()
        except Exception as e:
            result["kitti_shaped"] = {"skipped": repr(e)}


def leg_cpu_baseline_alone(C):
    # -------------------------------------------------- CPU baseline when the parity leg did not run (rank 0)
    # (main's locals this leg reads)
    args = getattr(C, 'args', None)
    ct = getattr(C, 'ct', None)
    cv = getattr(C, 'cv', None)
    i = getattr(C, 'i', None)
    k = getattr(C, 'k', None)
    kfs = getattr(C, 'kfs', None)
    n_poses = getattr(C, 'n_poses', None)
    ora = getattr(C, 'ora', None)
    oracle = getattr(C, 'oracle', None)
    oracle_lib = getattr(C, 'oracle_lib', None)
    rank = getattr(C, 'rank', None)
    result = getattr(C, 'result', None)
    t0 = getattr(C, 't0', None)
    vbx = getattr(C, 'vbx', None)
    world = getattr(C, 'world', None)
    if rank == 0 and world == 1 and not args.no_cpu_baseline and "cpu_baseline" not in result:
        from tests import oracle_lib
        oracle = oracle_lib.load()
        ora = oracle.voxblox(args.resolution) if vbx else oracle.chisel(args.resolution)
        nb = 400
        t0 = time.perf_counter()
        cv = 0
        for k in (kfs[i % n_poses] for i in range(nb)):
            if vbx:
                ora.integrate(k["xyz"], k["rgba"], k["Twc"])
            else:
                ora.integrate(k["xyz"], k["rgb"], k["kfid"], k["Twc"])
            cv += ora.last_visits()
        ct = time.perf_counter() - t0
        result["cpu_baseline"] = {
            "value": round(cv / ct / 1e6, 3), "unit": "Mvoxels/s", "cores": 1, "kind": "port",
            "sample": f"oracle/tsdf_{args.backend}.c (sequential / integrator_threads=1) on the first {nb} "
                      f"keyframes of the same stream, {ct:.1f} s, host has {os.cpu_count()} cores",
        }


def main():
    import types
    C = types.SimpleNamespace()
    args = parse()
    # ONE line on stdout: the compiled reference sources behind the cpu_baseline legs print (open_chisel a line per garbage
    # collection, line_descriptor a line per pyramid) — everything written to file descriptor 1 before the result goes to stderr
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
    # PLVS_BENCH_REHEARSAL=1 (scripts/gpu_check.sh, stage `multi` on a one-GPU box): every rank on device 0, the exchanges over
    # gloo (RCCL refuses two ranks on one device) — the N > 1 code path end to end with two real processes; never a measurement
    rehearsal = os.environ.get("PLVS_BENCH_REHEARSAL", "0") == "1"
    device_index = 0 if rehearsal else local_rank
    torch.cuda.set_device(device_index)
    multi = world > 1 or args.sharded_at_one
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if rehearsal:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank), rank=rank, world_size=world)

    from plvs_amd import _lib
    from tests.synth_scene import LOOP, make_keyframes, make_stream_keyframes
    from plvs_amd.shard import BlockDirectory, allgather_block_lists, sharded_integrate, sharded_integrate_voxblox
    from plvs_amd.tsdf import TsdfChisel, TsdfVoxblox

    # ---------------------------------------------------------------- inputs
    n_poses = 100                                    # 100 poses, 3.6 deg yaw step
    total_steps = args.warmup + args.steps
    vbx = args.backend == "voxblox"
    # N > 1 (voxblox, "simple"): the ray-sharded integrate of tsdf_voxblox_shard.hpp — rank r casts the rays of every N-th key
    # frame of the step and sends the voxel visits to the block owners.  STRONG scaling (the step stays --batch key frames):
    # the update is an ordered fold per voxel, and a step of N x 25 consecutive key frames of one camera makes every voxel's
    # run N times longer instead of giving the ranks more voxels (one device: 1.07 ms for 25 key frames, 21 ms for 200).
    vbx_sharded = multi and vbx
    if vbx:                      # 2 cm voxels, 16x12x3 m room, depths to 8 m
        if args.resolution == 0.05:
            args.resolution = 0.02
        if args.max_depth == 5.0:
            args.max_depth = 8.0
        if args.steady_state:
            kfs = make_keyframes(n_poses, room_size=(16.0, 12.0, 3.0), max_depth=args.max_depth, seed=0)
        else:      # the office stream from key frame 400 on, as the voxblox_configs3 leg of the default run
            n_poses = min(total_steps * args.batch, LOOP)
            kfs = make_stream_keyframes(n_poses, first=400, max_depth=args.max_depth, seed=0, threads=min(32, os.cpu_count() or 8))
        for k in kfs:
            k["rgba"] = np.concatenate([k["rgb"], np.full((k["rgb"].shape[0], 1), 255, np.uint8)], axis=1)
    elif args.steady_state:
        kfs = make_keyframes(n_poses, max_depth=args.max_depth, seed=0)
    # N > 1 (chisel, order-free): the ray-sharded integrate — rank r walks every N-th tile of the step's point
    # stream and sends what it collected to the chunk owners.  Weak scaling by default: a step carries --batch
    # keyframes PER GPU (a longer stretch of the stream, e.g. a map rebuild), so every rank's share of the rays
    # stays what one GPU walks at N = 1.
    ray_sharded = multi and not vbx and not args.ordered
    step_kfs = args.batch * (world if (ray_sharded and not args.strong) else 1)
    # N = 1, order-free chisel: the steps go in as the DEPTH IMAGES of the key frames (PLVS's real pipeline: depth image ->
    # GeneratePointCloudInCameraFrameBGRA -> InsertCloud); the same key frames as point streams stay in HBM for the other
    # legs (bit-exact mode, parity) and behind --cloud-input
    depth_input = not vbx and not multi and not args.ordered and not args.cloud_input
    if not vbx and not args.steady_state:
        # configs[2] stand-in, streaming: step s integrates key frames [s * step_kfs, (s + 1) * step_kfs) of the long
        # trajectory (tests/synth_scene.py: one loop of LOOP = 2500 DISTINCT key frames around a desk island in a
        # 9.5 x 7.5 x 3 m office; a job longer than the loop walks it again)
        n_poses = min(total_steps * step_kfs, LOOP)
        kfs = make_stream_keyframes(n_poses, max_depth=args.max_depth, seed=0, threads=min(32, os.cpu_count() or 8),
                                    images=depth_input)
    elif depth_input:
        kfs = make_keyframes(n_poses, max_depth=args.max_depth, seed=0, images=True)

    def pack_depth(sel, step=2):
        """The key frames as 640 x 480 images in HBM: depth and colour at the pixels of the stride-2 grid (the others are
        never read: src/PointCloudMapping.cc:957-996 visits m, n = 0, step, 2 step, ...), the grid table, one id per image."""
        gh, gw = sel[0]["depth_grid"].shape
        d = torch.zeros((len(sel), gh * step, gw * step), dtype=torch.float32, device="cuda")
        c = torch.zeros((len(sel), gh * step, gw * step, 3), dtype=torch.uint8, device="cuda")
        d[:, ::step, ::step] = torch.from_numpy(np.stack([k["depth_grid"] for k in sel])).cuda()
        c[:, ::step, ::step] = torch.from_numpy(np.stack([k["rgb_grid"] for k in sel])).cuda()
        return (d, c, torch.from_numpy(sel[0]["cam_grid"]).cuda(), step, 0.1, args.max_depth,
                torch.from_numpy(np.array([int(k["kfid"][0]) if len(k["kfid"]) else 0 for k in sel], np.int32)).cuda(),
                torch.from_numpy(np.stack([k["Twc"] for k in sel])).cuda())
    batches = []
    depth_batches = []
    built_depth = {}
    built = {}     # steps that carry the same key frames share one copy in HBM (at N x 100 key frames per step all do)
    for s in range(total_steps):
        first = (s * step_kfs) % n_poses
        if first not in built:
            sel = [kfs[(first + j) % n_poses] for j in range(step_kfs)]
            offsets = np.cumsum([0] + [k["xyz"].shape[0] for k in sel]).astype(np.int32)
            if depth_input and not args.full:     # (the point streams serve only the --full legs: kept off the device)
                built[first] = (None, None, None, offsets, None)
            else:
                xyz = torch.from_numpy(np.concatenate([k["xyz"] for k in sel])).cuda()
                rgb = torch.from_numpy(np.concatenate([k["rgba" if vbx else "rgb"] for k in sel])).cuda()
                kfid = torch.from_numpy(np.concatenate([k["kfid"] for k in sel]).astype(np.int32)).cuda()
                Twc = torch.from_numpy(np.stack([k["Twc"] for k in sel])).cuda()
                built[first] = (xyz, rgb, kfid, offsets, Twc)
            if depth_input:
                built_depth[first] = pack_depth(sel)
        batches.append(built[first])
        if depth_input:
            depth_batches.append(built_depth[first])

    if vbx:
        tsdf = TsdfVoxblox(args.resolution, max_blocks=65536, shard_rank=rank, shard_count=world)
    else:
        tsdf = TsdfChisel(args.resolution, max_chunks=16384, shard_rank=rank, shard_count=world,
                          order_free=not args.ordered)
    upd_cap = 16384          # = max_chunks: an updated-chunk list always fits
    d_upd = torch.zeros((upd_cap, 3), dtype=torch.int32, device="cuda")
    gathered_blocks = [0]
    gdir = BlockDirectory(16384) if multi else None      # every rank's copy of the global block -> owner table

    def step(b):
        if depth_input:      # b = (depth images, colour images, grid table, step, min, max, ids, poses), points of the step
            tsdf.integrate_depth_batch_dev(*b[0])
            st = tsdf.last_stats()
            st["points"] = b[1]          # (the library never forms the cloud: the points of the step from the generator)
            return st
        xyz, rgb, kfid, offsets, Twc = b
        if vbx_sharded:
            sharded_integrate_voxblox(tsdf, xyz, rgb, offsets, Twc)
        elif vbx:
            tsdf.integrate_batch_dev(xyz, rgb, offsets, Twc)
        elif ray_sharded:
            sharded_integrate(tsdf, xyz, rgb, kfid, offsets, Twc)
        else:
            tsdf.integrate_batch_dev(xyz, rgb, kfid, offsets, Twc)
        st = tsdf.last_stats()
        if multi:      # the updated block lists, over RCCL
            n = tsdf.updated_chunk_ids_dev(d_upd)
            all_ids, counts = allgather_block_lists(d_upd, n, upd_cap, padded=True)
            gdir.merge(all_ids, counts)
            gathered_blocks[0] += 1
        return st

    def barrier():
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    timed = [(depth_batches[s], int(batches[s][3][-1])) for s in range(total_steps)] if depth_input else batches
    for s in range(args.warmup):
        step(timed[s])
    if not vbx:
        tsdf.set_profiling(True)
    barrier()
    t0 = time.perf_counter()
    visits = 0
    points = 0
    max_run = 0
    voxels = 0
    step_wall = []
    for s in range(args.warmup, total_steps):
        ts0 = time.perf_counter()
        st = step(timed[s])
        step_wall.append(time.perf_counter() - ts0)   # (last_stats() has waited for the step: a per-step host clock)
        visits += st["visits"]
        points += st["points"]
        max_run = max(max_run, st["max_run"])
        voxels += st["voxels"]
    barrier()
    elapsed = time.perf_counter() - t0
    if vbx or ray_sharded:   # (the sharded step is three library calls around the exchanges: the wall clock is its time)
        stage_ms, calls = {}, args.steps
        if not vbx:
            tsdf.set_profiling(False)
    else:
        stage_ms, calls = tsdf.stage_ms()
        tsdf.set_profiling(False)
    if args.dump_outputs:
        dump_outputs(tsdf, args.dump_outputs if world == 1 else os.path.join(args.dump_outputs, f"rank{rank}"), st, vbx)

    # ---- N > 1 (ray-sharded): where a step's time goes, and the other scaling leg
    # phases_ms: three more steps run with a device synchronisation after each phase (walk / pack / exchange / apply /
    # feedback; max over ranks) — their sum exceeds ms_per_step by the overlap the synchronisations remove.
    # other_leg: the same job under the OTHER scaling rule (weak: --batch key frames per GPU per step; strong: --batch
    # key frames per step whatever N), so one run of `bench.py --gpus N` gives both curves.
    phases_ms, other_leg = None, None
    if vbx_sharded and args.full:
        tim = {}
        for s in range(3):
            sharded_integrate_voxblox(tsdf, *[batches[s % len(batches)][i] for i in (0, 1, 3, 4)], timings=tim)
        names = ["walk", "pack", "exchange", "apply"]
        t = torch.tensor([tim.get(k, 0.0) / 3.0 for k in names], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        phases_ms = {k: round(float(v), 4) for k, v in zip(names, t.tolist())}
    if ray_sharded and args.full:
        tim = {}
        for s in range(3):
            sharded_integrate(tsdf, *[batches[s % len(batches)][i] for i in (0, 1, 2, 3, 4)], timings=tim)
        names = ["walk", "pack", "exchange", "apply", "feedback"]
        t = torch.tensor([tim.get(k, 0.0) / 3.0 for k in names], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        phases_ms = {k: round(float(v), 4) for k, v in zip(names, t.tolist())}
        if world > 1 or os.environ.get("PLVS_BENCH_FORCE_OTHER_LEG"):   # (the variable: a one-GPU rehearsal of this branch)
            other_kfs = args.batch * (1 if not args.strong else world)
            sel = [kfs[j % n_poses] for j in range(other_kfs)]
            ob = (torch.from_numpy(np.concatenate([k["xyz"] for k in sel])).cuda(),
                  torch.from_numpy(np.concatenate([k["rgb"] for k in sel])).cuda(),
                  torch.from_numpy(np.concatenate([k["kfid"] for k in sel]).astype(np.int32)).cuda(),
                  np.cumsum([0] + [k["xyz"].shape[0] for k in sel]).astype(np.int32),
                  torch.from_numpy(np.stack([k["Twc"] for k in sel])).cuda())
            for s in range(max(args.warmup, 1)):
                step(ob)
            barrier()
            t1 = time.perf_counter()
            ov = 0
            for s in range(args.steps):
                ov += step(ob)["visits"]
            barrier()
            t = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            v = torch.tensor([ov], dtype=torch.int64, device="cuda")
            dist.all_reduce(v, op=dist.ReduceOp.SUM)
            other_leg = {"scaling": "strong" if not args.strong else "weak", "keyframes_per_step": other_kfs,
                         "value": round(int(v.item()) / float(t.item()) / 1e6, 2), "unit": "Mvoxels/s",
                         "ms_per_step": round(float(t.item()) / args.steps * 1e3, 3), "steps": args.steps}

    # max over ranks of the elapsed time, sum over ranks of the visits
    if multi:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        v = torch.tensor([visits], dtype=torch.int64, device="cuda")
        dist.all_reduce(v, op=dist.ReduceOp.SUM)
        visits_total = int(v.item())
    else:
        visits_total = visits

    result = None
    if rank == 0:
        mvox = visits_total / elapsed / 1e6
        # ------------------------------------------------------------ roofline
        # Algorithmic bytes: 32 B per voxel visit (16 B read + 16 B
        # written of logical payload) + 28 B per point, for what THIS rank applied.
        alg_bytes = (24.0 * visits + 16.0 * points) if vbx else (32.0 * visits + 28.0 * points)
        gpu_ms = sum(stage_ms.values()) if stage_ms else elapsed * 1e3
        dominant = max(stage_ms, key=stage_ms.get) if stage_ms else None
        achieved = alg_bytes / (gpu_ms * 1e-3) / 1e9 if gpu_ms > 0 else 0.0
        roofline = {
            "bound": "hbm", "achieved": round(achieved, 2), "peak": 8000.0, "unit": "GB/s",
            "frac": round(achieved / 8000.0, 5), "traffic": None,
            "kernel": f"tsdf_{args.backend} integrate pipeline (" + (", ".join(stage_ms) or "wall clock of the call") + ")",
            "ms_per_launch": round(gpu_ms / max(calls, 1), 4),
            "stage_ms_per_launch": {k: round(v / max(calls, 1), 4) for k, v in stage_ms.items()},
            "dominant_stage": dominant,
            "algorithmic_bytes_per_launch": alg_bytes / max(calls, 1),
        }
        # HBM bytes per launch from the PMC passes (FETCH_SIZE / WRITE_SIZE, separate rocprofv3
        # runs of this same command; scripts/pmc_traffic.py) committed under profiles/
        mode_tag = "" if vbx else ("_ordered" if args.ordered else "_order_free")
        # (the newest committed passes of this command: round 6's for the depth-image headline and the voxblox leg, round 5's /
        # round 4's where a later round made none)
        pdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
        rounds = ("r06", "r05") if depth_input else ("r06", "r04")
        pmc = ""
        for rr in rounds:
            pmc = os.path.join(pdir, f"{rr}_pmc_traffic_{args.backend}{mode_tag}{'_steady_state' if args.steady_state else ''}.json")
            if os.path.exists(pmc):
                break
        if world == 1 and not multi and args.batch == 100 and os.path.exists(pmc):
            with open(pmc) as f:
                t = json.load(f)
            roofline["traffic"] = t["traffic"]
            roofline["traffic_source"] = ("profiles/" + os.path.basename(pmc) + ": rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE "
                                          "passes of this command, FETCH_SIZE x2 (gfx950) + WRITE_SIZE, per launch")
        mode_name = "ordered (bit-exact)" if args.ordered else "order-free (fixed-point sums; sdf / weight within tolerance)"
        result = {
            "metric": ("Mvoxels/sec TSDF integrate (voxblox simple 2 cm / 8 m, 640x480 RGB-D)" if vbx else
                       "Mvoxels/sec TSDF integrate (chisel 5 cm / 5 m, 640x480 RGB-D)"),
            "value": round(mvox, 2), "unit": "Mvoxels/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak" if (ray_sharded and not args.strong) else "strong",
            "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": ("configs[3] stand-in: synthetic room 16x12x3 m, camera circle r=1 m, Voxblox "
                                    "simple TSDF 2 cm, max ray 5 m (wrapper constant), 76800-point keyframes" if vbx else
                                    ("configs[2] stand-in, STEADY STATE: synthetic room 6x4x3 m, camera circle r=1 m, every step "
                                     "re-integrates the same 100 key frames into a saturated map, Chisel TSDF 5 cm / 5 m, "
                                     "76800-point keyframes" if args.steady_state else
                                     "configs[2] stand-in, STREAMING: every step integrates the NEXT keyframes_per_step DISTINCT key "
                                     "frames of one 2500-key-frame loop around a desk island in a 9.5x7.5x3 m office (the shape of "
                                     "TUM fr3/long_office: 6 mm and 0.144 deg per key frame, new ground and revisits in every step, "
                                     "chunk allocation and colour folds inside the timed region), Chisel TSDF 5 cm / 5 m, 76800-pixel "
                                     "grid of which 36-73 k points per key frame have a depth below 5 m; the saturated-map figure of "
                                     "rounds 1-3 is the `steady_state` leg")),
                       "input": ("depth images (640x480, stride-2 grid): GeneratePointCloudInCameraFrameBGRA + InsertCloud fused, "
                                 "plvs_hip_tsdf_chisel_integrate_depth_batch_dev" if depth_input else
                                 "camera-frame point streams resident in HBM (integrate_batch_dev)"),
                       "mode": None if vbx else mode_name,
                       "resolution": args.resolution, "max_depth": args.max_depth,
                       "keyframes_per_step": step_kfs, "points_per_step": int(points // args.steps),
                       "ms_per_step_median_max": [round(float(np.median(step_wall)) * 1e3, 3), round(max(step_wall) * 1e3, 3)],
                       **({"ms_per_step_each": [round(x * 1e3, 2) for x in step_wall]} if multi else {}),
                       "visits_per_step": int(visits_total // args.steps),
                       "voxels_per_step": int(voxels // args.steps), "longest_voxel_run": int(max_run),
                       "parallelism": (f"ray-sharded x{world}: rank r walks tiles t = r (mod {world}), partial sums and "
                                       f"colour runs go to the chunk owners (three-prime hash mod {world}) in one "
                                       "all-to-all per step" if ray_sharded else
                                       (f"ray-sharded x{world}: rank r casts the rays of the key frames c = r (mod {world}), every voxel "
                                        f"visit goes to the block's owner (three-prime hash mod {world}) as a 16-byte record in one "
                                        "all-to-all per step, the owner applies them in the reference's order" if vbx_sharded else
                                        f"chunk-hash shard x{world}")),
                       "global_directory_blocks": (gdir.count() if gdir is not None else None)},
            "roofline": roofline,
        }
        if phases_ms is not None:
            result["phases_ms"] = phases_ms
        if other_leg is not None:
            result["other_scaling_leg"] = other_leg

    if args.full:      # every leg beside the headline
        C.__dict__.update(locals())   # (the leg reads main's locals through C)
        leg_realistic_calls(C)

        C.__dict__.update(locals())   # (the leg reads main's locals through C)
        leg_steady_state(C)

        C.__dict__.update(locals())   # (the leg reads main's locals through C)
        leg_other_chisel_mode(C)
        if hasattr(C, 't2'):
            t2 = C.t2

        C.__dict__.update(locals())   # (the leg reads main's locals through C)
        leg_parity_and_cpu_baseline(C)

        C.__dict__.update(locals())   # (the leg reads main's locals through C)
        leg_voxblox_configs3(C)

        C.__dict__.update(locals())   # (the leg reads main's locals through C)
        leg_frontend(C)

        C.__dict__.update(locals())   # (the leg reads main's locals through C)
        leg_cpu_baseline_alone(C)

    if rank == 0:
        try:      # (whatever the runtime's C libraries — RCCL's banner — still hold in stdio comes out BEFORE the line)
            import ctypes as _c
            _c.CDLL(None).fflush(None)
        except Exception:
            pass
        full = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_out")
        try:      # every leg with its prose (what each leg is: DESIGN.md §4.6)
            if args.full:
                os.makedirs(full, exist_ok=True)
                # (bench_full.json is the record of a --full run with the default sizes — every leg; a run with legs switched
                # off, another backend or other sizes — the profiling passes of scripts/ — writes bench_partial.json and
                # leaves it alone)
                whole = not (args.no_other_mode_leg or args.no_voxblox_leg or args.no_realistic_legs or args.no_steady_state_leg or
                             args.no_frontend or args.no_cpu_baseline or args.no_parity_check or args.steady_state or args.ordered or
                             args.cloud_input or args.sharded_at_one or args.backend != "chisel" or world != 1 or args.batch != 100)
                result["legs_present"] = sorted(k for k in result if isinstance(result[k], dict) and k not in ("config", "roofline"))
                with open(os.path.join(full, "bench_full.json" if whole else "bench_partial.json"), "w") as f:
                    json.dump(result, f, indent=1)
        except OSError:
            pass
        sys.stdout.flush()
        ctypes.CDLL(None).fflush(None)
        os.dup2(real_stdout, 1)
        print(json.dumps(result if args.verbose_line else compact_line(result)), flush=True)
    tsdf.close()
    if multi:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
