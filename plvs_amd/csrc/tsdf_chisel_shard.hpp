// Host side of the ray-sharded multi-GPU integrate (kernels: tsdf_shard.hpp).  A step is three calls per rank:
//   shard_walk   the rank walks its share of the call's tiles (tile t belongs to rank t % N) through every chunk they
//                cross, sorts the segments by chunk and sums them per voxel into one send region per owning rank;
//   shard_pack   copies the regions and the runs into the caller's send buffers (the exchange is the caller's);
//   shard_apply  the owner applies what it received as the order-free integrate applies its own segments, and folds the
//                colours through the received runs.
#pragma once
#include "tsdf_chisel_order_free.hpp"
#include "tsdf_chisel_halo.hpp"
#include "tsdf_shard.hpp"

namespace {

// The start of shard_apply in one launch: counters of the call cleared, the received totals in place (what a
// handful of small memsets / copies would do, each a runtime call of its own).
__global__ void shard_apply_begin(Counters* ctr, WalkCounters* wctr, int32_t* xcount_sat, uint32_t* __restrict__ chunk_nseg,
                                  uint32_t max_chunks, uint32_t total_seg, uint32_t total_runs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t c = i; c < max_chunks; c += gridDim.x * blockDim.x) chunk_nseg[c] = 0u;
  if (i == 0) {
    ctr->total_visits = 0u;
    ctr->err = 0u; ctr->num_heads = 0u; ctr->num_updated = 0u; ctr->max_run = 0u; ctr->num_desc = 0u;
    wctr[0] = WalkCounters{};
    wctr[1] = WalkCounters{};
    wctr[0].seg_top = total_seg;
    wctr[1].num_desc = total_runs;
    *xcount_sat = 0;
  }
}

}  // namespace

static int shard_state_init(plvs_tsdf_chisel* h) {
  if (h->xdir.keys) return PLVS_OK;
  // the walk directory: every chunk of the whole map may pass through it (ids + 512 B of bits each)
  const size_t xmax = std::min<size_t>((size_t)h->prm.max_chunks * (size_t)std::max(1, h->prm.shard_count), (size_t)1 << 22);
  size_t cap = 1024;
  while (cap < 2 * xmax) cap <<= 1;
  h->xdir.mask = (uint32_t)(cap - 1);
  h->xdir.max_blocks = (int32_t)xmax;
  PLVS_HIP_TRY(hipMalloc((void**)&h->xdir.keys, cap * sizeof(unsigned long long)));
  PLVS_HIP_TRY(hipMalloc((void**)&h->xdir.slots, cap * sizeof(int32_t)));
  PLVS_HIP_TRY(hipMalloc((void**)&h->xdir.slot_ids, xmax * 3 * sizeof(int32_t)));
  PLVS_HIP_TRY(hipMalloc((void**)&h->x_sat, xmax * (kChunkVox / 32) * sizeof(uint32_t)));
  PLVS_HIP_TRY(hipMalloc((void**)&h->d_xcount, 4 * sizeof(int32_t)));   // [0] chunks, [1] error bits, [2] saturated this call
  PLVS_HIP_TRY(hipHostMalloc((void**)&h->h_sh_counts, ((size_t)3 * 64 + 2) * sizeof(long long)));
  PLVS_HIP_TRY(hipHostMalloc((void**)&h->h_sh_ctl, 320 * sizeof(uint32_t)));
  PLVS_HIP_TRY(hipHostMalloc((void**)&h->h_sh_off, (128 + 132) * sizeof(uint32_t)));
  PLVS_HIP_TRY(hipMemset(h->xdir.keys, 0xFF, cap * sizeof(unsigned long long)));
  PLVS_HIP_TRY(hipMemset(h->xdir.slots, 0xFF, cap * sizeof(int32_t)));
  PLVS_HIP_TRY(hipMemset(h->x_sat, 0, xmax * (kChunkVox / 32) * sizeof(uint32_t)));
  PLVS_HIP_TRY(hipMemset(h->d_xcount, 0, 4 * sizeof(int32_t)));
  return PLVS_OK;
}

static int shard_state_clear(plvs_tsdf_chisel* h) {
  if (!h->xdir.keys) return PLVS_OK;
  const size_t cap = (size_t)h->xdir.mask + 1;
  PLVS_HIP_TRY(hipMemset(h->xdir.keys, 0xFF, cap * sizeof(unsigned long long)));
  PLVS_HIP_TRY(hipMemset(h->xdir.slots, 0xFF, cap * sizeof(int32_t)));
  PLVS_HIP_TRY(hipMemset(h->x_sat, 0, (size_t)h->xdir.max_blocks * (kChunkVox / 32) * sizeof(uint32_t)));
  PLVS_HIP_TRY(hipMemset(h->d_xcount, 0, 4 * sizeof(int32_t)));
  h->sh_phase = 0;
  h->sh_nsat = 0;
  h->sh_wait_first = h->sh_wait_count = 0;
  return PLVS_OK;
}

// The rank's share of a call's tiles: tile t of the stream is local tile t / N of rank t % N.
static TileMap shard_tile_map(const plvs_tsdf_chisel* h) {
  const int N = std::max(1, h->prm.shard_count);
  return TileMap{(uint32_t)N, N > 1 ? (uint32_t)h->prm.shard_rank : 0u};
}

// ---- shard_walk

// One shard_walk call: the caller's inputs and what its stages share.
struct ShardWalk {
  const float* d_xyz;
  int n, nclouds;
  int N;              // ranks
  uint32_t nt;        // tiles of this rank
  size_t xmax;        // capacity of the walk directory
  WalkScratch scratch;
  AccOut out;         // (of the attempt under way)
};

// The call checked, its tile table filled and on the device, the rank's tiles and points counted.
static int shard_walk_begin(plvs_tsdf_chisel* h, const int32_t* offsets, int nclouds, int64_t* send_counts, hipStream_t s,
                            ShardWalk* c) {
  const int N = std::max(1, h->prm.shard_count), rank = N > 1 ? h->prm.shard_rank : 0;
  for (int p = 0; p < 3 * N; ++p) send_counts[p] = 0;
  h->sh_stats = plvs_tsdf_stats{};
  h->sh_phase = 0;
  int n = 0;
  int rc = check_offsets(offsets, nclouds, &n);
  if (rc == PLVS_OK) rc = shard_state_init(h);
  if (rc != PLVS_OK) return rc;
  for (int p = 0; p < 3 * N; ++p) h->h_sh_counts[p] = 0;
  h->sh_n = n;
  h->sh_nclouds = nclouds;
  h->sh_tiletab.resize(2 * ((size_t)nclouds + 1));
  h->sh_ntiles = plvs::tsdf::fill_tile_table(offsets, nclouds, h->sh_tiletab.data(), kWalkRays);   // (tiles never straddle clouds)
  if (h->sh_ntiles >= (1u << kWireTileBits)) {
    plvs::set_error("tsdf_chisel shard_walk: %u tiles in one call exceed the wire format's tile index (split the batch)", h->sh_ntiles);
    return PLVS_ERR_CAPACITY;
  }
  h->sh_nt = 0;
  h->sh_runs = 0;
  h->sh_phase = 1;
  int64_t own = 0;   // the points of this rank's tiles
  for (int cl = 0; cl < nclouds; ++cl) {
    const uint32_t t0 = (uint32_t)h->sh_tiletab[(size_t)nclouds + 1 + cl], t1 = (uint32_t)h->sh_tiletab[(size_t)nclouds + 2 + cl];
    for (uint32_t t = t0; t < t1; ++t)
      if (t % (uint32_t)N == (uint32_t)rank)
        own += std::min<int64_t>(kWalkRays, (int64_t)(offsets[cl + 1] - offsets[cl]) - (int64_t)(t - t0) * kWalkRays);
  }
  h->sh_stats.points = own;
  // (the tile table goes to the device even on a rank without tiles: the runs other ranks send it name tiles of the stream)
  PLVS_HIP_TRY(h->offsets.reserve(2 * ((size_t)nclouds + 1)));
  PLVS_HIP_TRY(hipMemcpyAsync(h->offsets.p, h->sh_tiletab.data(), 2 * ((size_t)nclouds + 1) * sizeof(int32_t),
                              hipMemcpyHostToDevice, s));
  c->n = n;
  c->nclouds = nclouds;
  c->N = N;
  c->nt = h->sh_ntiles > (uint32_t)rank ? (h->sh_ntiles - (uint32_t)rank + (uint32_t)N - 1u) / (uint32_t)N : 0u;
  c->xmax = (size_t)h->xdir.max_blocks;
  return PLVS_OK;
}

// The poses on the device, and what a walk of nt tiles needs whatever its attempt.
static int shard_walk_reserve(plvs_tsdf_chisel* h, ShardWalk& c, const float* d_Twc, hipStream_t s) {
  const size_t xmax = c.xmax;
  const uint32_t nt = c.nt;
  PLVS_HIP_TRY(h->poses.reserve((size_t)c.nclouds));
  hipLaunchKernelGGL(pose_prep, dim3(ceil_div((size_t)c.nclouds, 64)), dim3(64), 0, s, d_Twc, c.nclouds, h->poses.p);
  int rc = reserve_chunk_tables(h, xmax, (uint32_t)std::min<size_t>(xmax, 64));
  if (rc != PLVS_OK) return rc;
  PLVS_HIP_TRY(h->w_seg_cnt.reserve(nt));
  PLVS_HIP_TRY(h->w_tile_visits.reserve(nt));
  PLVS_HIP_TRY(h->w_deferred.reserve(nt));   // (one list: a single lean pass)
  PLVS_HIP_TRY(h->w_run_cnt.reserve(nt));
  PLVS_HIP_TRY(h->w_run_off.reserve((size_t)nt + 1));
  PLVS_HIP_TRY(h->sh_nrec.reserve(xmax));
  PLVS_HIP_TRY(h->sh_owner.reserve(xmax));
  PLVS_HIP_TRY(h->sh_slot_owner.reserve(xmax));
  PLVS_HIP_TRY(h->sh_run_ctr.reserve((size_t)3 * 64));   // counts, bases, fill cursors per destination
  PLVS_HIP_TRY(h->sh_ctl.reserve(256 + 2));              // regions, fill cursors, region totals
  c.scratch = walk_scratch(h, nt);
  return PLVS_OK;
}

// One attempt's walk: the rank's tiles through every chunk they cross (the walk directory), lean kernel first, the
// general one for what it deferred.
static int shard_walk_launch(plvs_tsdf_chisel* h, ShardWalk& c, hipStream_t s) {
  const uint32_t nt = c.nt;
  int rc = reserve_walk_scratch(h, nt, c.scratch);
  if (rc != PLVS_OK) return rc;
  const size_t run_slots = (size_t)nt << h->run_r1_log2;   // (what follows grows to twice a call's need as well)
  if (h->dkey0.cap < run_slots) PLVS_HIP_TRY(h->dkey0.reserve(2 * run_slots));   // (all a call's runs, whatever their number)
  if (h->sh_run_first.cap < run_slots) PLVS_HIP_TRY(h->sh_run_first.reserve(2 * run_slots));   // (first wire record per run)
  if (h->w_val0.cap < run_slots) PLVS_HIP_TRY(h->w_val0.reserve(2 * run_slots));
  PLVS_HIP_TRY(h->scratch.reserve(scan_scratch_words(nt)));
  PLVS_HIP_TRY(hipMemsetAsync(h->d_wctr, 0, 2 * sizeof(WalkCounters), s));
  PLVS_HIP_TRY(hipMemsetAsync(h->w_chunk_nseg.p, 0, c.xmax * sizeof(uint32_t), s));
  PLVS_HIP_TRY(hipMemsetAsync(h->sh_run_ctr.p, 0, 3 * 64 * sizeof(uint32_t), s));
  Params Pw = h->P;       // this rank walks its tiles through every chunk they cross
  Pw.shard_count = 1;
  Pw.shard_rank = 0;
  const TileMap tmap = shard_tile_map(h);
  c.out = walk_out(h, c.scratch, nullptr);   // (nullptr: seg_pass<false> counts the chunks' segments)
  const RunOut runs{h->w_runkey.p, h->w_masks.p, h->w_run_cnt.p, h->run_r1_log2};
  // (a chunk entered by an attempt that has to be repeated stays in the walk directory: harmless)
  hipLaunchKernelGGL(walk_fast<kFastEntries>, dim3(nt), dim3(kWalkRays), 0, s, Pw, h->scale_u, h->scale_w, c.d_xyz, c.n,
                     h->offsets.p, c.nclouds, h->poses.p, h->xdir, h->d_xcount, h->d_wctr, (const uint32_t*)nullptr,
                     (const uint32_t*)h->x_sat, c.out, runs, tmap, (uint32_t)kWalkLimit, (const uint32_t*)nullptr,
                     (const uint32_t*)nullptr, h->w_deferred.p, &h->d_wctr->ndeferred, (const GridSrc*)nullptr);
  hipLaunchKernelGGL((walk_tiles<true, true>), dim3(kDeferGrid), dim3(kWalkRays), 0, s, Pw, h->scale_u, h->scale_w, c.d_xyz, c.n,
                     h->offsets.p, c.nclouds, h->poses.p, h->xdir, h->d_xcount, h->d_wctr, (const uint32_t*)nullptr,
                     (const uint32_t*)h->x_sat, c.out, runs, tmap, (uint32_t)nt, (const uint32_t*)h->w_deferred.p,
                     (const uint32_t*)&h->d_wctr->ndeferred, (uint32_t)kWalkLimit,
                     1u, (const GridSrc*)nullptr);   // (flagged = overflowed 2048 entries: this kernel's table takes 3584, the tile goes whole)
  return PLVS_OK;
}

// Behind the segment sort: the send regions planned per destination, the runs listed densely in tile order and counted
// per destination; the region sizes and the walk's counters published and read (h_plan: descriptors, records).
static int shard_walk_plan(plvs_tsdf_chisel* h, const ShardWalk& c, uint32_t* h_plan, hipStream_t s) {
  const int N = c.N;
  const uint32_t nt = c.nt;
  hipLaunchKernelGGL(shard_chunk_totals, dim3(1024), dim3(256), 0, s, h->w_sorted_seg.p, h->updated.p,
                     h->w_active_off.p, h->xdir.slot_ids, N, h->d_wctr, h->sh_nrec.p, h->sh_owner.p, h->sh_slot_owner.p);
  hipLaunchKernelGGL(shard_plan, dim3(1), dim3(1024), 0, s, h->sh_nrec.p, h->sh_owner.p, N, h->d_wctr, h->sh_ctl.p,
                     h->sh_ctl.p + 256);
  // the runs, densely, in tile order (seg_scan has left their number in num_desc), counted per destination
  PLVS_HIP_TRY(exclusive_scan_u32(h->w_run_cnt.p, h->w_run_off.p, nt, nullptr, h->scratch.p, s));
  hipLaunchKernelGGL(compact_runs, dim3(ceil_div(nt, 4)), dim3(256), 0, s, h->w_runkey.p, h->w_run_cnt.p,
                     h->w_run_off.p, nt, h->run_r1_log2, h->dkey0.p, h->w_val0.p, no_guard());
  hipLaunchKernelGGL(shard_run_count, dim3(2048), dim3(256), 0, s, h->dkey0.p, h->w_val0.p, &h->d_wctr[0].num_desc,
                     h->w_masks.p, h->sh_slot_owner.p, N, h->sh_run_ctr.p, h->sh_run_first.p, h->d_wctr);
  hipLaunchKernelGGL(shard_run_plan, dim3(1), dim3(64), 0, s, h->sh_run_ctr.p, N, h->d_wctr);
  PLVS_KERNEL_CHECK();
  // sizes of the send regions (and whether the walk has to be repeated)
  hipLaunchKernelGGL(publish_words, dim3(1), dim3(64), 0, s, (const uint32_t*)(h->sh_ctl.p + 256), h_plan, 2,
                     reinterpret_cast<const uint32_t*>(h->d_wctr), reinterpret_cast<uint32_t*>(h->h_wctr),
                     (int)(sizeof(WalkCounters) / sizeof(uint32_t)), (const uint32_t*)nullptr, (uint32_t*)nullptr, 0);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(hipStreamSynchronize(s));
  return PLVS_OK;
}

// This rank's own aggregation: one sum per touched voxel into the owner's send region; the regions' fill and the run
// counts published and read.
static int shard_walk_aggregate(plvs_tsdf_chisel* h, const uint32_t* h_plan, hipStream_t s) {
  PLVS_HIP_TRY(h->sh_seg_reg.reserve(2 * (size_t)h_plan[0] + 2));
  PLVS_HIP_TRY(h->sh_rec_reg.reserve(2 * (size_t)h_plan[1] + 2));
  uint32_t* const ctl = h->sh_ctl.p;
  launch_apply<false, true>(h, h->w_rec.p, nullptr,
                            EmitOut{h->xdir.slot_ids, h->sh_owner.p, ctl, ctl + 64, ctl + 128, ctl + 192, h->sh_seg_reg.p,
                                    h->sh_rec_reg.p}, 0u, s);
  PLVS_KERNEL_CHECK();
  hipLaunchKernelGGL(publish_words, dim3(1), dim3(256), 0, s, (const uint32_t*)h->sh_ctl.p, h->h_sh_ctl, 256,
                     (const uint32_t*)h->sh_run_ctr.p, h->h_sh_ctl + 256, 64, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(hipStreamSynchronize(s));
  return PLVS_OK;
}

// What the caller's exchange needs (per destination: descriptors, records, runs), room for the next call's chunks
// applied in parts, the stats.
static int shard_walk_finish(plvs_tsdf_chisel* h, const ShardWalk& c, int64_t* send_counts) {
  for (int p = 0; p < c.N; ++p) {
    h->h_sh_counts[3 * p] = (long long)h->h_sh_ctl[128 + p];
    h->h_sh_counts[3 * p + 1] = (long long)h->h_sh_ctl[192 + p];
    h->h_sh_counts[3 * p + 2] = (long long)h->h_sh_ctl[256 + p];
  }
  if (h->h_wctr->num_multi > h->multi_cap) {
    int rc = ensure_part_acc(h, (uint32_t)std::min<size_t>(c.xmax, (size_t)h->h_wctr->num_multi + h->h_wctr->num_multi / 2));
    if (rc != PLVS_OK) return rc;
  }
  h->sh_runs = h->h_wctr->num_desc;
  for (int p = 0; p < 3 * c.N; ++p) send_counts[p] = (int64_t)h->h_sh_counts[p];
  h->sh_stats.visits = (int64_t)h->h_wctr->total_visits;
  return PLVS_OK;
}

// ---- shard_apply

// One shard_apply call: the caller's inputs, the received totals.
struct ShardApply {
  const void *d_seg_src, *d_rec_src, *d_run_src;
  const uint8_t* d_rgb;
  const uint32_t* d_kfid;
  int N, max_chunks;
  size_t tseg, trec, trun;   // received descriptors, records, runs
  int chunks_before;
  uint32_t* d_src_off;       // (device) where each rank's descriptors and records start in the receive buffers
};

// The receive counts checked and turned into offsets (pinned: h_sh_off + 128, 2 (N + 1) <= 130 words).
static int shard_apply_check(plvs_tsdf_chisel* h, const int64_t* recv_counts, ShardApply* c) {
  const int N = c->N;
  PLVS_REQUIRE(h->h_sh_off != nullptr, "shard_apply follows shard_walk");
  uint32_t* const src_off = h->h_sh_off + 128;
  size_t tseg = 0, trec = 0, trun = 0;
  for (int q = 0; q < N; ++q) {
    PLVS_REQUIRE(recv_counts[3 * q] >= 0 && recv_counts[3 * q + 1] >= 0 && recv_counts[3 * q + 2] >= 0, "negative receive count");
    src_off[q] = (uint32_t)tseg;
    src_off[N + 1 + q] = (uint32_t)trec;
    tseg += (size_t)recv_counts[3 * q];
    trec += (size_t)recv_counts[3 * q + 1];
    trun += (size_t)recv_counts[3 * q + 2];
  }
  src_off[N] = (uint32_t)tseg;
  src_off[2 * N + 1] = (uint32_t)trec;
  PLVS_REQUIRE(tseg < 0x7FFFFFFFull && trec < 0xFFFFFFFFull && trun < 0x7FFFFFFFull,
               "receive buffers beyond the index range (split the batch)");
  c->tseg = tseg;
  c->trec = trec;
  c->trun = trun;
  return PLVS_OK;
}

static int shard_apply_reserve(plvs_tsdf_chisel* h, const ShardApply& c) {
  const uint32_t total = (uint32_t)c.tseg;
  PLVS_HIP_TRY(h->sh_src_off.reserve(128 + 132));
  PLVS_HIP_TRY(h->w_seg.reserve(2 * (size_t)total));
  PLVS_HIP_TRY(h->w_sorted_seg.reserve(2 * (size_t)total));
  // every chunk applied in parts has more than kPartMin segments: the received total bounds their number
  return reserve_chunk_tables(h, (size_t)c.max_chunks,
                              std::min<uint32_t>((uint32_t)c.max_chunks, total / std::max(1u, h->part_min) + 1u));
}

// The counters of the call cleared and the received totals in place; the received descriptors translated to this rank's
// pool slots (first-touch chunks created) and sorted by chunk.  The walk ran in shard_walk: its stage time stays 0 here.
static int shard_apply_sort(plvs_tsdf_chisel* h, ShardApply& c, hipStream_t s) {
  const uint32_t total = (uint32_t)c.tseg;
  c.chunks_before = h->num_chunks;
  c.d_src_off = h->sh_src_off.p + 128;   // (apart from the words shard_pack's kernels may still be reading)
  PLVS_HIP_TRY(hipMemcpyAsync(c.d_src_off, h->h_sh_off + 128, 2 * ((size_t)c.N + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(shard_apply_begin, dim3(ceil_div((size_t)c.max_chunks, 1024)), dim3(256), 0, s, h->d_ctr, h->d_wctr,
                     h->d_xcount + 2, h->w_chunk_nseg.p, (uint32_t)c.max_chunks, total, (uint32_t)c.trun);
  PLVS_HIP_TRY(stage_mark(h, 0, s));
  PLVS_HIP_TRY(stage_mark(h, 1, s));
  hipLaunchKernelGGL(shard_translate, dim3(ceil_div((size_t)total, 256)), dim3(256), 0, s,
                     static_cast<const uint4*>(c.d_seg_src), total, c.d_src_off, c.N, h->dir, &h->d_ctr->num_chunks,
                     &h->d_wctr[0].err, h->w_seg.p);
  sort_segments(h, SegSrc{(size_t)total, total, 0u, nullptr},
                SegScan{&h->d_ctr->num_chunks, c.max_chunks, nullptr, nullptr, 0u, nullptr}, s);
  PLVS_HIP_TRY(stage_mark(h, 2, s));
  return PLVS_OK;
}

// Colours: the received runs, by (voxel, tile), folded as the order-free integrate folds its own.
static int shard_apply_colours(plvs_tsdf_chisel* h, const ShardApply& c, hipStream_t s) {
  const uint32_t R = (uint32_t)c.trun;
  const uint32_t* runs = static_cast<const uint32_t*>(c.d_run_src);
  PLVS_HIP_TRY(h->dkey0.reserve(R));
  PLVS_HIP_TRY(h->dkey1.reserve(R));
  PLVS_HIP_TRY(h->w_val0.reserve(R));
  PLVS_HIP_TRY(h->w_val1.reserve(R));
  PLVS_HIP_TRY(h->sh_vkey.reserve(R));
  PLVS_HIP_TRY(h->heads.reserve(R));
  PLVS_HIP_TRY(h->sh_sat.reserve(R));
  PLVS_HIP_TRY(h->w_dummy.reserve((size_t)c.max_chunks + 1));
  PLVS_HIP_TRY(h->scratch.reserve(radix_scratch_words(R)));
  uint32_t* const err = &h->d_wctr[0].err;
  hipLaunchKernelGGL(shard_run_translate, dim3(ceil_div((size_t)R, 256)), dim3(256), 0, s, runs, R, h->dir, err,
                     h->sh_vkey.p, h->dkey0.p, h->w_val0.p);
  int tile_bits = 1;
  while ((1ull << tile_bits) < (unsigned long long)h->sh_ntiles) ++tile_bits;
  bool second = false;
  PLVS_HIP_TRY(radix_sort_pairs(h->dkey0.p, h->w_val0.p, h->dkey1.p, h->w_val1.p, R, 0, tile_bits, h->scratch.p, s, &second));
  uint32_t* order = second ? h->w_val1.p : h->w_val0.p;
  uint32_t* other = second ? h->w_val0.p : h->w_val1.p;
  uint32_t* k_in = second ? h->dkey0.p : h->dkey1.p;   // the key buffer the tile sort has left free
  uint32_t* k_out = second ? h->dkey1.p : h->dkey0.p;
  hipLaunchKernelGGL(shard_gather_keys, dim3(ceil_div((size_t)R, 256)), dim3(256), 0, s, h->sh_vkey.p, order, R, k_in);
  // (a received descriptor can add one chunk at most: the chunks before the call + the descriptors bound the slots)
  const long long slot_bound = std::min<long long>(c.max_chunks, (long long)c.chunks_before + (long long)c.tseg);
  PLVS_HIP_TRY(radix_sort_pairs(k_in, order, k_out, other, R, 0, voxel_key_bits(slot_bound), h->scratch.p, s, &second));
  const uint32_t* skeys = second ? k_out : k_in;
  const uint32_t* sval = second ? other : order;
  hipLaunchKernelGGL(voxel_heads, dim3(ceil_div(R, 256 * kHeadTiles)), dim3(256), 0, s, skeys, R, h->heads.p,
                     h->w_dummy.p, h->d_wctr + 1);
  hipLaunchKernelGGL(fold_colours_masks<false>, dim3(std::min<size_t>(ceil_div(R, kFoldWaves), 8192)), dim3(64 * kFoldWaves), 0, s,
                     skeys, sval, &h->d_wctr[1].num_desc,
                     RunSrc{runs, kWireRun, 0u, TileMap{1u, 0u}, h->offsets.p, h->sh_nclouds, nullptr}, h->heads.p, c.d_rgb,
                     h->rgbw, &h->d_wctr[1].num_heads, h->sh_sat.p, reinterpret_cast<uint32_t*>(h->d_xcount + 2),
                     (const uint32_t*)nullptr, GridSrc{});
  PLVS_KERNEL_CHECK();
  return PLVS_OK;
}

// The finished call: the saturated voxels' count and the counters read, the stats, the stage times.
static int shard_apply_finish(plvs_tsdf_chisel* h, const ShardApply& c, hipStream_t s) {
  hipLaunchKernelGGL(publish_words, dim3(1), dim3(64), 0, s, reinterpret_cast<const uint32_t*>(h->d_xcount + 2),
                     reinterpret_cast<uint32_t*>(h->h_sh_counts), 1, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0,
                     (const uint32_t*)nullptr, (uint32_t*)nullptr, 0);
  int rc = read_walk_counters(h, s);
  if (rc != PLVS_OK) return rc;
  if (h->h_wctr->err) return walk_fail(h, h->h_wctr->err);
  h->sh_nsat = (uint32_t)(*reinterpret_cast<int32_t*>(h->h_sh_counts));
  h->num_chunks = h->h_ctr->num_chunks;
  h->stats.new_chunks = h->num_chunks - c.chunks_before;
  h->stats.updated_chunks = (int32_t)h->h_wctr->num_updated;
  h->stats.voxels = (int32_t)h->h_wctr->num_heads;
  h->stats.max_run = (int32_t)h->h_wctr->max_run;
  h->last_updated = h->h_wctr->num_updated;
  if (h->profiling) {
    if ((rc = add_stage_times(h, 0, kWalkStages)) != PLVS_OK) return rc;
    h->prof_calls++;
  }
  return PLVS_OK;
}

extern "C" {

int plvs_hip_tsdf_chisel_shard_walk(plvs_tsdf_chisel* h, const float* d_xyz, const int32_t* offsets, int nclouds,
                                    const float* d_Twc, int64_t* send_counts, void* stream) {
  PLVS_REQUIRE(h && send_counts, "null argument");
  PLVS_REQUIRE(!h->poisoned, "handle is in a failed state (clear it)");
  PLVS_REQUIRE(h->prm.order_free != 0 && h->prm.shard_count >= 1 && h->prm.shard_count <= 64,
               "the ray-sharded integrate needs order_free = 1 and 1 <= shard_count <= 64");
  PLVS_REQUIRE(offsets && nclouds >= 0, "bad offsets");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ShardWalk c{};
  c.d_xyz = d_xyz;
  int rc = shard_walk_begin(h, offsets, nclouds, send_counts, s, &c);
  if (rc != PLVS_OK || c.nt == 0) return rc;
  PLVS_REQUIRE(d_xyz && d_Twc, "null device pointer");
  h->sh_nt = c.nt;
  if ((rc = shard_walk_reserve(h, c, d_Twc, s)) != PLVS_OK) return rc;
  uint32_t* const h_plan = reinterpret_cast<uint32_t*>(h->h_sh_counts + 3 * 64);
  for (int attempt = 0;; ++attempt) {
    if ((rc = shard_walk_launch(h, c, s)) != PLVS_OK) return rc;
    sort_segments(h, SegSrc{c.scratch.seg_own + c.scratch.seg_spill, c.out.seg_cap, c.nt, h->w_seg_cnt.p},
                  SegScan{h->d_xcount, (int)c.xmax, h->w_tile_visits.p, h->w_run_cnt.p, c.nt, nullptr}, s);
    if ((rc = shard_walk_plan(h, c, h_plan, s)) != PLVS_OK) return rc;
    const uint32_t err = h->h_wctr->err;
    if (err & kErrPoolFull) {
      plvs::set_error("tsdf_chisel shard_walk: the walk directory is full (max_chunks x shard_count chunks)");
      return poisoned(h);
    }
    if (err & ~kErrScratch) return walk_fail(h, err);
    if (!(err & kErrScratch)) break;
    if (attempt >= 8 || !grow_walk_scratch(h, c.nt, c.scratch)) return walk_fail(h, err);
  }
  if ((rc = shard_walk_aggregate(h, h_plan, s)) != PLVS_OK) return rc;
  return shard_walk_finish(h, c, send_counts);
}

int plvs_hip_tsdf_chisel_shard_pack(plvs_tsdf_chisel* h, void* d_seg_dst, void* d_rec_dst, void* d_run_dst, void* stream) {
  PLVS_REQUIRE(h, "null handle");
  PLVS_REQUIRE(h->sh_phase == 1, "shard_pack follows shard_walk");
  hipStream_t s = static_cast<hipStream_t>(stream);
  h->sh_phase = 2;
  const int N = std::max(1, h->prm.shard_count);
  long long nseg = 0;
  for (int p = 0; p < N; ++p) nseg += h->h_sh_counts ? h->h_sh_counts[3 * p] : 0;
  if (nseg == 0) return PLVS_OK;
  PLVS_REQUIRE(d_seg_dst && d_rec_dst && (h->sh_runs == 0 || d_run_dst), "null send buffer");
  // (pinned staging: the copy is asynchronous and its source outlives this call; the previous step's copies have
  // executed — shard_apply ends with a synchronisation)
  uint32_t* const dst_off = h->h_sh_off;
  for (int p = 0; p < 128; ++p) dst_off[p] = 0;
  for (int p = 1; p < N; ++p) {
    dst_off[p] = dst_off[p - 1] + (uint32_t)h->h_sh_counts[3 * (p - 1)];
    dst_off[64 + p] = dst_off[64 + p - 1] + (uint32_t)h->h_sh_counts[3 * (p - 1) + 1];
  }
  PLVS_HIP_TRY(h->sh_src_off.reserve(128 + 132));
  PLVS_HIP_TRY(hipMemcpyAsync(h->sh_src_off.p, dst_off, 128 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(shard_copy_regions, dim3(512), dim3(256), 0, s, h->sh_seg_reg.p, h->sh_rec_reg.p, h->sh_ctl.p,
                     h->sh_src_off.p, N, static_cast<uint4*>(d_seg_dst), static_cast<uint4*>(d_rec_dst));
  if (h->sh_runs > 0)
    hipLaunchKernelGGL(shard_run_pack, dim3(std::min<size_t>(ceil_div((size_t)h->sh_runs, kRunSpan), 4096)), dim3(256), 0, s,
                       h->dkey0.p, h->w_val0.p, &h->d_wctr[0].num_desc, h->w_masks.p, h->sh_run_first.p, h->run_r1_log2,
                       shard_tile_map(h), h->xdir.slot_ids, h->sh_slot_owner.p, h->sh_run_ctr.p + 64, h->sh_run_ctr.p + 128, static_cast<uint32_t*>(d_run_dst));
  PLVS_KERNEL_CHECK();
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_shard_apply(plvs_tsdf_chisel* h, const void* d_seg_src, const void* d_rec_src,
                                     const void* d_run_src, const int64_t* recv_counts, const uint8_t* d_rgb,
                                     const uint32_t* d_kfid, void* stream) {
  PLVS_REQUIRE(h && recv_counts, "null argument");
  PLVS_REQUIRE(!h->poisoned, "handle is in a failed state (clear it)");
  PLVS_REQUIRE(h->sh_phase == 2, "shard_apply follows shard_pack");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = halo_drop(h, s);   // first-touch chunks go into the pool slots a meshing halo may still occupy
  if (rc != PLVS_OK) return rc;
  h->sh_phase = 0;
  h->sh_nsat = 0;
  ShardApply c{d_seg_src, d_rec_src, d_run_src, d_rgb, d_kfid, std::max(1, h->prm.shard_count), h->prm.max_chunks};
  if ((rc = shard_apply_check(h, recv_counts, &c)) != PLVS_OK) return rc;
  h->stats = h->sh_stats;
  h->last_updated = 0;
  h->stage_set = 1;
  if (c.tseg == 0) return PLVS_OK;
  PLVS_REQUIRE(d_seg_src && d_rec_src && d_rgb && (c.trun == 0 || d_run_src), "null device pointer");
  if ((rc = shard_apply_reserve(h, c)) != PLVS_OK) return rc;
  if ((rc = shard_apply_sort(h, c, s)) != PLVS_OK) return rc;
  launch_apply<true, false>(h, static_cast<const uint4*>(d_rec_src), d_kfid, EmitOut{}, 0u, s);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(stage_mark(h, 3, s));
  if (c.trun > 0 && (rc = shard_apply_colours(h, c, s)) != PLVS_OK) return rc;
  PLVS_HIP_TRY(stage_mark(h, 4, s));
  return shard_apply_finish(h, c, s);
}

int plvs_hip_tsdf_chisel_shard_saturated(plvs_tsdf_chisel* h, int32_t* d_voxels, int cap, int* n, void* stream) {
  PLVS_REQUIRE(h && n, "null argument");
  *n = (int)h->sh_nsat;
  if (h->sh_nsat == 0) return PLVS_OK;
  if (cap < (int)h->sh_nsat) {
    plvs::set_error("shard_saturated: %u voxels, room for %d", h->sh_nsat, cap);
    return PLVS_ERR_CAPACITY;
  }
  PLVS_REQUIRE(d_voxels, "null output");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(shard_saturated_ids, dim3(ceil_div((size_t)h->sh_nsat, 256)), dim3(256), 0, s, h->sh_sat.p, h->sh_nsat,
                     h->dir.slot_ids, d_voxels);
  PLVS_KERNEL_CHECK();
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_shard_saturated_message(plvs_tsdf_chisel* h, int32_t* d_msg, int rows, void* stream) {
  PLVS_REQUIRE(h && d_msg && rows > 0, "bad argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->sh_nsat > 0) {   // the last shard_apply's voxels join the waiting list
    const size_t need = 4 * ((size_t)h->sh_wait_first + h->sh_wait_count + h->sh_nsat);
    if (need > h->sh_wait.cap) {
      DevBuf<int32_t> grown;
      PLVS_HIP_TRY(grown.reserve(need));
      if (h->sh_wait_count)
        PLVS_HIP_TRY(hipMemcpyAsync(grown.p, h->sh_wait.p + 4 * (size_t)h->sh_wait_first, 16 * (size_t)h->sh_wait_count,
                                    hipMemcpyDeviceToDevice, s));
      PLVS_HIP_TRY(hipStreamSynchronize(s));
      h->sh_wait.release();
      h->sh_wait = grown;
      h->sh_wait_first = 0;
    }
    hipLaunchKernelGGL(shard_saturated_ids, dim3(ceil_div((size_t)h->sh_nsat, 256)), dim3(256), 0, s, h->sh_sat.p, h->sh_nsat,
                       h->dir.slot_ids, h->sh_wait.p + 4 * ((size_t)h->sh_wait_first + h->sh_wait_count));
    h->sh_wait_count += h->sh_nsat;
    h->sh_nsat = 0;
  }
  const uint32_t k = std::min<uint32_t>(h->sh_wait_count, (uint32_t)rows);
  hipLaunchKernelGGL(shard_sat_message, dim3(std::max<unsigned>(1u, ceil_div((size_t)k, 256))), dim3(256), 0, s,
                     h->sh_wait.p ? h->sh_wait.p + 4 * (size_t)h->sh_wait_first : (const int32_t*)nullptr, k, (uint32_t)rows, d_msg);
  PLVS_KERNEL_CHECK();
  h->sh_wait_first += k;
  h->sh_wait_count -= k;
  if (h->sh_wait_count == 0) h->sh_wait_first = 0;
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_shard_note_gathered(plvs_tsdf_chisel* h, const int32_t* d_gathered, int nranks, int rows, void* stream) {
  PLVS_REQUIRE(h && d_gathered && nranks >= 1 && rows > 0, "bad argument");
  PLVS_REQUIRE(h->prm.order_free != 0 && h->prm.shard_count >= 1, "not a ray-sharded map");
  int rc = shard_state_init(h);
  if (rc != PLVS_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(shard_note_gathered, dim3(ceil_div((size_t)rows, 256), (unsigned)nranks), dim3(256), 0, s, d_gathered,
                     (uint32_t)rows, h->xdir, h->d_xcount, reinterpret_cast<uint32_t*>(h->d_xcount + 1), h->x_sat);
  PLVS_KERNEL_CHECK();
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_shard_note_saturated(plvs_tsdf_chisel* h, const int32_t* d_voxels, int n, void* stream) {
  PLVS_REQUIRE(h && n >= 0, "bad argument");
  PLVS_REQUIRE(h->prm.order_free != 0 && h->prm.shard_count >= 1, "not a ray-sharded map");
  if (n == 0) return PLVS_OK;
  PLVS_REQUIRE(d_voxels, "null list");
  int rc = shard_state_init(h);
  if (rc != PLVS_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(shard_note_saturated, dim3(ceil_div((size_t)n, 256)), dim3(256), 0, s, d_voxels, (uint32_t)n, h->xdir,
                     h->d_xcount, reinterpret_cast<uint32_t*>(h->d_xcount + 1), h->x_sat);
  PLVS_KERNEL_CHECK();
  return PLVS_OK;
}

}  // extern "C"
