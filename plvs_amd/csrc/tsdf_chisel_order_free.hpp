// Order-free mode of the open_chisel back end (order_free = 1): the single-walk pipeline of tsdf_walk.hpp — walk_tiles ->
// segment sort -> apply_chunks, and the colour fold for the voxels whose colour weight is below 254.  sdf / weight within a
// stated float tolerance of the reference's sequential loop, kfid and colour exact.  The plan of a call is
// tsdf_walk_plan.hpp's; this file reserves, launches what a plan says, and reads the outcome.  The launches of segment
// sort and apply stage, and the walk's scratch, serve the ray-sharded integrate as well (tsdf_chisel_shard.hpp).
#pragma once
#include "tsdf_chisel_handle.hpp"

namespace {

// The order-free call's whole prologue in one launch: poses, the cloud offsets (read from the pinned host copy),
// zeroed counters and per-chunk segment counts.  (Seven small commands — copy, kernel, five fills — cost 40 us of
// queueing in front of a 55 us walk of one keyframe.)
__global__ void walk_prologue(const float* __restrict__ Twc, int nclouds, Pose* __restrict__ poses,
                              const int32_t* __restrict__ host_offsets, int32_t* __restrict__ offsets,
                              WalkCounters* __restrict__ wctr, Counters* __restrict__ ctr, uint32_t* __restrict__ chunk_nseg,
                              int nseg, int ntile_first = 0) {
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  for (int c = i0; c < nclouds; c += stride) make_pose(Twc + 12 * c, &poses[c]);
  // (offsets + tile table, and behind them the first point of every tile: what the colour fold reads per run)
  for (int c = i0; c < 2 * (nclouds + 1) + ntile_first; c += stride) offsets[c] = host_offsets[c];
  for (int k = i0; k < nseg; k += stride) chunk_nseg[k] = 0u;
  uint32_t* w = reinterpret_cast<uint32_t*>(wctr);
  for (int k = i0; k < (int)(2 * sizeof(WalkCounters) / sizeof(uint32_t)); k += stride) w[k] = 0u;
  if (i0 == 0) {   // reset the per-call counters, keep num_chunks
    ctr->total_visits = 0;
    ctr->err = 0;
    ctr->num_heads = 0;
    ctr->num_updated = 0;
    ctr->max_run = 0;
    ctr->num_desc = 0;
  }
}

}  // namespace

// ------------------------------------------------------------------ single-walk pipeline (tsdf_walk.hpp)
constexpr unsigned kDeferGrid = 1024;   // workgroups of the general walk over the deferred tiles (it loops over the list)
// The lean walk comes with three table sizes (tsdf_walk.hpp, FastShared): 2048 entries at two tiles per CU for a call that
// fills the device, 4096 entries at one tile per CU for the tiles that overflowed 2048 — a dozen in a hundred on an office
// scene with points up to 5 m away — and for every tile of a call of at most kSmallCallTiles tiles (a few key frames: one
// tile per CU is all there is to run, and a deferral costs such a call a second walk's latency); and the small table of
// the first pass over near surfaces, kFastEntriesSmall (tsdf_walk.hpp) = 1536 entries at three tiles per CU.  A tile owns
// kRecStride records (the larger table's limit) in the record buffer.
// The plan (tsdf_walk_plan.hpp) names a pass by its table CLASS: `entries` 1024 = the small class, whatever the small
// table's size has become — launch_walk_passes launches the kFastEntriesSmall instance for it.
constexpr int kPlanSmallClass = 1024, kFastEntries = 2048, kFastEntriesBig = 4096;
static_assert(kFastEntriesSmall > kPlanSmallClass && kFastEntriesSmall < kFastEntries, "the small table lies between its class name and the next table");
constexpr uint32_t kRecStride = kFastEntriesBig * 7 / 8;
static_assert(kRecStride == (uint32_t)kWalkLimit, "a tile's record region holds a flush of the largest table");
static_assert(kSortSmallRuns == kSmallRuns && kSortMediumRuns <= kMediumRuns && kCollectPartRuns == kCollectPart &&
                  kRowsPerChunk == (uint32_t)kSlabs && kTileSegments == (uint32_t)kWalkChunks && kSegmentBlock == (uint32_t)kSegSpan,
              "tsdf_walk_plan.hpp plans for the kernels' sizes");

// compact_runs for a call whose runs the host knows: no bound, nothing to pad.
static RunGuard no_guard() { return RunGuard{0xFFFFFFFFu, nullptr, nullptr, 0, nullptr, nullptr, 0u, nullptr, 0u}; }

// Stable sort of the D runs walk_tiles left in the per-tile regions by voxel key: per voxel its runs
// in tile (= point) order; the value carried is the run's slot (tile = slot >> r1_log2, mask at slot * 8).
static int sort_runs(plvs_tsdf_chisel* h, uint32_t D, uint32_t ntiles, int num_chunks, hipStream_t s,
                     const uint32_t** skeys, const uint32_t** sval, const RunGuard* guard = nullptr) {
  // guard (a chain launched before the host knows the call's runs): D and num_chunks are BOUNDS, compact_runs pads the pairs
  // up to D and leaves the verdict in *guard->skip
  PLVS_HIP_TRY(h->dkey0.reserve(D));
  PLVS_HIP_TRY(h->dkey1.reserve(D));
  PLVS_HIP_TRY(h->w_val0.reserve(D));
  PLVS_HIP_TRY(h->w_val1.reserve(D));
  PLVS_HIP_TRY(h->w_run_off.reserve((size_t)ntiles + 1));
  PLVS_HIP_TRY(h->scratch.reserve(std::max(radix_scratch_words(D), scan_scratch_words(ntiles))));
  // (the caller has scanned run_cnt into w_run_off)
  // (the count after this call's insertions; + 1 under a guard: its padding keys, all ones, must not be a voxel's)
  const int key_bits = voxel_key_bits((long long)num_chunks + (guard ? 1 : 0));
  // (the plain sort of a known number of pairs: its status words are zeroed by the compaction, on the side — a launch of its
  // own otherwise, 25 us in front of the chain)
  const size_t zero_words = guard ? 0 : radix_sort_zero_words(D, 0, key_bits);
  RunGuard g = guard ? *guard : no_guard();
  g.zero = zero_words ? h->scratch.p : nullptr;
  g.zero_words = (uint32_t)zero_words;
  hipLaunchKernelGGL(compact_runs, dim3(ceil_div(ntiles, 4) + (guard ? std::min<unsigned>(64u, ceil_div((size_t)D, 1024)) : 0u)),
                     dim3(256), 0, s, h->w_runkey.p, h->w_run_cnt.p, h->w_run_off.p, ntiles, h->run_r1_log2, h->dkey0.p,
                     h->w_val0.p, g);
  bool second = false;
  if (zero_words)
    PLVS_HIP_TRY(radix_sort_pairs_zeroed(h->dkey0.p, h->w_val0.p, h->dkey1.p, h->w_val1.p, D, 0, key_bits, h->scratch.p, s,
                                         &second));
  else
    PLVS_HIP_TRY(radix_sort_pairs(h->dkey0.p, h->w_val0.p, h->dkey1.p, h->w_val1.p, D, 0, key_bits, h->scratch.p, s,
                                  &second));
  *skeys = second ? h->dkey1.p : h->dkey0.p;
  *sval = second ? h->w_val1.p : h->w_val0.p;
  return PLVS_OK;
}

// Accumulators for `chunks` chunks applied in parts (apply_chunks leaves them zero).
static int ensure_part_acc(plvs_tsdf_chisel* h, uint32_t chunks) {
  if (chunks <= h->multi_cap) return PLVS_OK;
  const size_t nv = (size_t)chunks * kChunkVox, nd = (size_t)chunks * kSlabs;
  h->pa_wuu.release(); h->pa_w.release(); h->pa_last.release(); h->pa_cnt.release(); h->pa_done.release();
  h->multi_cap = 0;
  PLVS_HIP_TRY(h->pa_wuu.reserve(nv));
  PLVS_HIP_TRY(h->pa_w.reserve(nv));
  PLVS_HIP_TRY(h->pa_last.reserve(nv));
  PLVS_HIP_TRY(h->pa_cnt.reserve(nv));
  PLVS_HIP_TRY(h->pa_done.reserve(nd));
  PLVS_HIP_TRY(hipMemset(h->pa_wuu.p, 0, nv * sizeof(long long)));
  PLVS_HIP_TRY(hipMemset(h->pa_w.p, 0, nv * sizeof(unsigned long long)));
  PLVS_HIP_TRY(hipMemset(h->pa_last.p, 0, nv * sizeof(uint32_t)));
  PLVS_HIP_TRY(hipMemset(h->pa_cnt.p, 0, nv * sizeof(uint32_t)));
  PLVS_HIP_TRY(hipMemset(h->pa_done.p, 0, nd * sizeof(uint32_t)));
  h->multi_cap = chunks;
  return PLVS_OK;
}

// The per-chunk tables of segment sort and apply stage for a directory of `chunks` slots (the pool's max_chunks; the walk
// directory's capacity for a sharded walk), and accumulators for part_chunks chunks applied in parts.
static int reserve_chunk_tables(plvs_tsdf_chisel* h, size_t chunks, uint32_t part_chunks) {
  PLVS_HIP_TRY(h->w_chunk_nseg.reserve(chunks));
  PLVS_HIP_TRY(h->w_chunk_off.reserve(chunks + 1));
  PLVS_HIP_TRY(h->w_chunk_fill.reserve(chunks));
  PLVS_HIP_TRY(h->w_active_off.reserve(chunks + 1));
  PLVS_HIP_TRY(h->updated.reserve(chunks + 1));
  PLVS_HIP_TRY(h->w_part_off.reserve(chunks + 1));
  PLVS_HIP_TRY(h->w_multi_idx.reserve(chunks + 1));
  return ensure_part_acc(h, part_chunks);
}

// ---- segment sort (w_seg -> w_sorted_seg, by chunk) and apply stage: seg_pass<false> counts the chunks' segments where the
// walk has not (AccOut::chunk_nseg), seg_scan scans and lists the updated chunks, seg_pass<true> places.  Where the walk
// has counted them, every segment holds a ticket and seg_place — or runs_count — places it without counting again.

// The descriptor slots a pass looks at: the tiles' own regions and the spill area behind them (walk_out), or a dense list
// of seg_cap descriptors (ntiles = 0, no seg_cnt).
struct SegSrc {
  size_t slots;
  uint32_t seg_cap, ntiles;
  const uint32_t* seg_cnt;
};
template <bool kScatter>
static void launch_seg_pass(plvs_tsdf_chisel* h, const SegSrc& src, hipStream_t q) {
  hipLaunchKernelGGL((seg_pass<kScatter>), dim3(ceil_div(src.slots, kSegSpan)), dim3(256), 0, q, h->w_seg.p, src.seg_cap,
                     src.ntiles, src.seg_cnt, h->w_chunk_nseg.p, h->w_chunk_off.p, h->w_chunk_fill.p, h->w_sorted_seg.p,
                     h->d_wctr);
}
// The place of the walk's ticketed segments in chunk order (w_sorted_seg holds two uint4 per segment).
static SegPlace seg_place_args(const plvs_tsdf_chisel* h, uint32_t seg_cap) {
  return SegPlace{h->w_seg_ticket.p, h->w_chunk_off.p, h->w_sorted_seg.p, (uint32_t)std::min<size_t>(h->w_sorted_seg.cap / 2, 0xFFFFFFFFu),
                  seg_cap};
}
static void launch_seg_place(plvs_tsdf_chisel* h, const SegSrc& src, hipStream_t q) {
  const SegPlace a = seg_place_args(h, src.seg_cap);
  hipLaunchKernelGGL(seg_place, dim3(ceil_div(src.slots, 256)), dim3(256), 0, q, h->w_seg.p, a.ticket, src.seg_cap, src.ntiles,
                     src.seg_cnt, a.chunk_off, a.sorted, a.sorted_cap, h->d_wctr);
}

// num_chunks / chunk_cap: the directory the segments' slots belong to; tile_visits, run_cnt: per tile, summed on the way
// (null: a list of received segments); active_idx: chunk slot -> place among the updated, for the collected chain.
struct SegScan {
  const int32_t* num_chunks;
  int chunk_cap;
  const uint32_t *tile_visits, *run_cnt;
  uint32_t ntiles;
  uint32_t* active_idx;
};
static void launch_seg_scan(plvs_tsdf_chisel* h, const SegScan& a, hipStream_t q) {
  hipLaunchKernelGGL(seg_scan, dim3(1), dim3(1024), 0, q, h->w_chunk_nseg.p, h->w_chunk_off.p, h->w_chunk_fill.p, h->updated.p,
                     h->w_active_off.p, h->d_wctr, a.num_chunks, a.chunk_cap, a.tile_visits, a.run_cnt, a.ntiles,
                     h->w_part_off.p, h->w_multi_idx.p, h->multi_cap, h->part_segs, h->part_min, a.active_idx);
}

// All three, for segments nobody has counted yet (the ray-sharded integrate).
static void sort_segments(plvs_tsdf_chisel* h, const SegSrc& src, const SegScan& scan, hipStream_t q) {
  launch_seg_pass<false>(h, src, q);
  launch_seg_scan(h, scan, q);
  launch_seg_pass<true>(h, src, q);
}

// The apply stage over the sorted segments; kWide, kEmit, last_shift: apply_chunks (tsdf_walk.hpp).  kEmit: the sums leave
// for the chunks' owners (emit) and the map is not touched.
template <bool kWide, bool kEmit>
static void launch_apply(plvs_tsdf_chisel* h, const uint4* rec, const uint32_t* d_kfid, const EmitOut& emit, uint32_t last_shift,
                         hipStream_t q) {
  hipLaunchKernelGGL((apply_chunks<kWide, kEmit>), dim3(4096), dim3(kApplyThreads), 0, q, h->w_sorted_seg.p, h->updated.p,
                     h->w_active_off.p, h->w_part_off.p, h->w_multi_idx.p, h->part_segs,
                     PartAcc{h->pa_wuu.p, h->pa_w.p, h->pa_last.p, h->pa_cnt.p, h->pa_done.p}, rec,
                     kEmit ? 0.0 : 1.0 / (double)h->scale_u, kEmit ? 0.0 : 1.0 / (double)h->scale_w, d_kfid,
                     kEmit ? (float*)nullptr : h->sdf, kEmit ? (float*)nullptr : h->weight, kEmit ? (uint32_t*)nullptr : h->kfid,
                     h->d_wctr, emit, last_shift);
}

// The walk's scratch (integrate_walk_acc, shard_walk): every tile owns kRecStride records, kWalkChunks segments and
// 2^run_r1_log2 run slots; what a tile has beyond its own goes to a spill area behind the tiles' regions.  A walk that runs
// out of any of them sets kErrScratch and leaves the map untouched: the regions grow and the call is repeated.
struct WalkScratch {
  size_t rec_own, seg_own, rec_spill, seg_spill;
};
static WalkScratch walk_scratch(const plvs_tsdf_chisel* h, uint32_t ntiles) {
  WalkScratch w;
  w.rec_own = (size_t)ntiles * kRecStride;
  w.seg_own = (size_t)ntiles * kWalkChunks;
  w.rec_spill = std::max<size_t>(h->w_rec.cap > w.rec_own ? h->w_rec.cap - w.rec_own : 0, (size_t)1 << 16);
  w.seg_spill = std::max<size_t>(h->w_seg.cap / 2 > w.seg_own ? h->w_seg.cap / 2 - w.seg_own : 0, (size_t)1 << 12);
  return w;
}
static int reserve_walk_scratch(plvs_tsdf_chisel* h, uint32_t ntiles, const WalkScratch& w) {
  // (sized by the call's tiles, and the largest buffers of the handle — 64 B of masks per run slot, hundreds of MB: a
  // hipFree + hipMalloc of that size costs milliseconds, and a stream of calls of varying length would pay it whenever a
  // call is a little longer than any before; they grow to TWICE what a call needs instead)
  if (h->w_rec.cap < w.rec_own + w.rec_spill) PLVS_HIP_TRY(h->w_rec.reserve(2 * w.rec_own + w.rec_spill));
  if (h->w_seg.cap < 2 * (w.seg_own + w.seg_spill)) PLVS_HIP_TRY(h->w_seg.reserve(2 * (2 * w.seg_own + w.seg_spill)));
  PLVS_HIP_TRY(h->w_sorted_seg.reserve(h->w_seg.cap));
  PLVS_HIP_TRY(h->w_seg_ticket.reserve(h->w_seg.cap / 2));
  const size_t run_slots = (size_t)ntiles << h->run_r1_log2;
  if (h->w_runkey.cap < run_slots) {
    PLVS_HIP_TRY(h->w_runkey.reserve(2 * run_slots));
    PLVS_HIP_TRY(h->w_masks.reserve(2 * run_slots * kMaskWords));
  }
  PLVS_HIP_TRY(h->w_masks.reserve(run_slots * kMaskWords));
  return PLVS_OK;
}
static AccOut walk_out(const plvs_tsdf_chisel* h, const WalkScratch& w, uint32_t* chunk_nseg) {
  return AccOut{h->w_rec.p, (uint32_t)std::min<size_t>(w.rec_own + w.rec_spill, 0xFFFFFFFFu), h->w_seg.p,
                (uint32_t)std::min<size_t>(w.seg_own + w.seg_spill, 0xFFFFFFFFu), h->w_seg_cnt.p, h->w_tile_visits.p, chunk_nseg,
                chunk_nseg ? h->w_seg_ticket.p : nullptr};
}
// kErrScratch: room for twice what the walk asked for (h_wctr).  false: the tiles' run slots would leave the index range.
static bool grow_walk_scratch(plvs_tsdf_chisel* h, uint32_t ntiles, WalkScratch& w) {
  w.rec_spill = std::max<size_t>(w.rec_spill, (size_t)h->h_wctr->rec_top * 2);
  w.seg_spill = std::max<size_t>(w.seg_spill, (size_t)h->h_wctr->seg_top * 2);
  while ((1u << h->run_r1_log2) < h->h_wctr->run_need) ++h->run_r1_log2;
  return ((size_t)ntiles << h->run_r1_log2) < 0xFFFFFFFFull;
}

// ---- Order-free mode: walk_tiles -> segment sort -> apply_chunks (+ the colour fold when the call met voxels whose colour
// weight is below 254).  The policy — which passes, which colour chain, which stream — is plan_walk_call's
// (tsdf_walk_plan.hpp); the functions below launch what a plan says.

// One attempt of a call: the caller's inputs and what its stages share.
struct WalkCall {
  const float* d_xyz;
  const uint8_t* d_rgb;
  const uint32_t* d_kfid;
  int n, nclouds;
  uint32_t ntiles;
  int max_chunks;
  const GridSrc* gsrc;     // depth-image entry: the host's copy of the grid description (null: point clouds) ...
  const GridSrc* d_grid;   //   ... and the device's, behind the offsets
  size_t seg_slots;        // the tiles' segment slots and the spill area behind them
  AccOut out;
  RunOut runs;
  const uint32_t* last_count;   // (device) tiles the last lean pass left to walk_tiles
  uint32_t collect_seq;         // kChainCollected: the sequence number rows_place publishes the walk's counters under
};

template <int E>
static void launch_walk_fast(plvs_tsdf_chisel* h, const WalkCall& c, const WalkPass& pass, hipStream_t s) {
  uint32_t* const counts[3] = {&h->d_wctr->ndeferred, &h->d_wctr->ndeferred2, &h->d_wctr->ndeferred3};
  const uint32_t* const list = pass.src < 0 ? nullptr : h->w_deferred.p + (size_t)pass.src * c.ntiles;
  const uint32_t* const nlist = pass.src < 0 ? nullptr : counts[pass.src];
  // (the direct and the list form are two kernels — walk_fast's kList; the small table is a first pass only, its list
  // form is not built: launch_walk_passes)
  constexpr bool kHasList = E != kFastEntriesSmall;
  const bool listed = kHasList && list != nullptr;
  const auto kernel = c.d_grid ? (listed ? walk_fast<E, true, kHasList> : walk_fast<E, true, false>)
                               : (listed ? walk_fast<E, false, kHasList> : walk_fast<E, false, false>);
  hipLaunchKernelGGL(kernel, dim3(pass.grid), dim3(kWalkRays), 0, s, h->P, h->scale_u, h->scale_w, c.d_xyz, c.n, h->offsets.p,
                     c.nclouds, h->poses.p, h->dir, &h->d_ctr->num_chunks, h->d_wctr, h->rgbw, (const uint32_t*)nullptr, c.out,
                     c.runs, TileMap{1u, 0u, 1u}, kRecStride, list, nlist, h->w_deferred.p + (size_t)pass.dst * c.ntiles,
                     counts[pass.dst], c.d_grid);
}

// The common case of a tile alone in a lean kernel; what the passes defer (tiles over several clouds, table overflows) is
// walked by the general kernel from the last pass's list.
static void launch_walk_passes(plvs_tsdf_chisel* h, const WalkPlan& plan, const WalkCall& c, hipStream_t s) {
  for (int i = 0; i < plan.npasses; ++i) {
    const WalkPass& pass = plan.pass[i];
    // (the plan's 1024 is the small CLASS, not a size: see kPlanSmallClass; the plan gives it every tile — a list would
    // go to the next table, which holds whatever the small one does: the same records either way)
    if (pass.entries == kPlanSmallClass && pass.src < 0) launch_walk_fast<kFastEntriesSmall>(h, c, pass, s);
    else if (pass.entries == kFastEntries || pass.entries == kPlanSmallClass) launch_walk_fast<kFastEntries>(h, c, pass, s);
    else launch_walk_fast<kFastEntriesBig>(h, c, pass, s);
  }
  hipLaunchKernelGGL((walk_tiles<true, true>), dim3(kDeferGrid), dim3(kWalkRays), 0, s, h->P, h->scale_u, h->scale_w, c.d_xyz,
                     c.n, h->offsets.p, c.nclouds, h->poses.p, h->dir, &h->d_ctr->num_chunks, h->d_wctr, h->rgbw,
                     (const uint32_t*)nullptr, c.out, c.runs, TileMap{1u, 0u, 1u}, c.ntiles,
                     (const uint32_t*)(h->w_deferred.p + (size_t)plan.last_list * c.ntiles), c.last_count, kRecStride,
                     plan.pieces, c.d_grid);
}

// Segment sort and apply stage on stream q; in front of them, for a call whose runs may be collected chunk by chunk, the
// colour side's counting stages: short kernels that would otherwise start beside the apply stage's first thousand
// workgroups and wait for their slots (40 us each, measured).
static int segments_and_apply(plvs_tsdf_chisel* h, const WalkPlan& plan, const WalkCall& c, hipStream_t q) {
  launch_seg_scan(h, SegScan{&h->d_ctr->num_chunks, c.max_chunks, h->w_tile_visits.p, h->w_run_cnt.p, c.ntiles,
                             plan.collect_ready ? h->w_active_idx.p : nullptr}, q);
  if (plan.collect_ready) {
    const bool queued = plan.chain == kChainCollected;   // (rows_place then publishes the walk's counters for the host)
    PLVS_HIP_TRY(hipStreamWaitEvent(q, h->ev_zero, 0));
    hipLaunchKernelGGL(runs_count, dim3(plan.collect_blocks), dim3(kSegSpan), 0, q, h->w_seg.p, h->w_rseg.p, c.ntiles, h->w_seg_cnt.p,
                       h->w_active_idx.p, plan.collect_rows, plan.collect_blocks, h->w_run_matrix.p, h->w_rpre.p, h->d_wctr, c.last_count,
                       seg_place_args(h, c.out.seg_cap));
    hipLaunchKernelGGL(runs_rowscan, dim3(std::min<uint32_t>(ceil_div(plan.collect_rows, 4), 1024u)), dim3(256), 0, q,
                       h->w_run_matrix.p, plan.collect_rows, plan.collect_blocks, h->d_wctr, h->w_item_cnt.p);
    hipLaunchKernelGGL(rows_place, dim3(1), dim3(1024), 0, q, h->w_item_cnt.p, plan.collect_rows, plan.collect_bound,
                       (uint32_t)std::min<size_t>(plan.parts_cap, 0xFFFFFFFFu), h->d_wctr,
                       h->w_item_base.p, h->w_item_part0.p, h->w_part_item.p, reinterpret_cast<const uint32_t*>(h->d_ctr),
                       reinterpret_cast<uint32_t*>(h->h_wctr), reinterpret_cast<uint32_t*>(h->h_ctr),
                       (uint32_t)(sizeof(Counters) / sizeof(uint32_t)), queued ? h->h_seq : (uint32_t*)nullptr,
                       queued ? c.collect_seq : 0u);
    PLVS_HIP_TRY(hipEventRecord(h->ev_seg, q));
  }
  // (the walk has ticketed its segments: runs_count has placed them on its way, whatever the chain then does; no launch
  // between the counting stages and the apply stage)
  if (!plan.collect_ready) launch_seg_place(h, SegSrc{c.seg_slots, c.out.seg_cap, c.ntiles, h->w_seg_cnt.p}, q);
  PLVS_HIP_TRY(stage_mark(h, 2, q));
  launch_apply<false, false>(h, h->w_rec.p, c.d_kfid, EmitOut{}, c.gsrc ? c.gsrc->key_bits : 0u, q);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(stage_mark(h, 3, q));
  return PLVS_OK;
}

// The colour fold: the truncating u8 mean is order dependent -> through the sorted runs of the voxels whose colour weight
// is below 254 (D of them, or a bound: `skip` then says whether the chain in front held).
static int launch_fold(plvs_tsdf_chisel* h, const WalkCall& c, uint32_t D, const uint32_t* skeys, const uint32_t* sval,
                       const uint32_t* skip, hipStream_t q) {
  const RunSrc rsrc{h->w_masks.p, (uint32_t)kMaskWords, h->run_r1_log2, TileMap{1u, 0u}, h->offsets.p, c.nclouds,
                    reinterpret_cast<const uint32_t*>(h->offsets.p) + 2 * ((size_t)c.nclouds + 1)};
  const auto kernel = c.gsrc ? fold_colours_masks<true> : fold_colours_masks<false>;
  hipLaunchKernelGGL(kernel, dim3(std::min<size_t>(ceil_div(D, kFoldWaves), 8192)), dim3(64 * kFoldWaves), 0, q, skeys, sval,
                     &h->d_wctr[1].num_desc, rsrc, h->heads.p, c.d_rgb, h->rgbw, &h->d_wctr[1].num_heads, (uint32_t*)nullptr,
                     (uint32_t*)nullptr, skip, c.gsrc ? *c.gsrc : GridSrc{});
  PLVS_KERNEL_CHECK();
  return PLVS_OK;
}

// One workgroup, one launch: the runs listed, sorted and their voxels' first runs found.
template <int BITS>
static void launch_sort_medium(plvs_tsdf_chisel* h, uint32_t ntiles, int passes, const RunGuard* guard, hipStream_t q) {
  hipLaunchKernelGGL(sort_runs_medium<BITS>, dim3(1), dim3(1024), 0, q, h->w_runkey.p, h->w_run_cnt.p, ntiles, h->run_r1_log2,
                     h->d_wctr + 1, h->dkey0.p, h->w_val0.p, h->dkey1.p, h->w_val1.p, h->w_run_off.p, h->heads.p, passes,
                     guard ? guard->limit : 0xFFFFFFFFu, &h->d_ctr->num_chunks, guard ? guard->chunk_limit : 0,
                     guard ? guard->skip : (uint32_t*)nullptr);
}

// The sorting colour chain for D runs in a map of `chunks` chunks — or bounds on both (guard) — on stream q.  Where
// sort_needs_scan(D, ntiles), the caller has queued the scan of the run counts in front of it.
static int colour_chain(plvs_tsdf_chisel* h, const WalkCall& c, uint32_t D, int chunks, const RunGuard* guard, hipStream_t q) {
  const uint32_t* skeys = h->dkey0.p;
  const uint32_t* sval = h->w_val0.p;
  switch (sort_kind(D, c.ntiles)) {
    case kSortSmall:
      hipLaunchKernelGGL(sort_runs_small, dim3(1), dim3(1024), 0, q, h->w_runkey.p, h->w_run_cnt.p, c.ntiles,
                         h->run_r1_log2, h->d_wctr + 1, h->dkey0.p, h->w_val0.p, h->heads.p, guard ? guard->skip : (uint32_t*)nullptr);
      break;
    case kSortMedium: {
      PLVS_HIP_TRY(h->dkey0.reserve(D));
      PLVS_HIP_TRY(h->dkey1.reserve(D));
      PLVS_HIP_TRY(h->w_val0.reserve(D));
      PLVS_HIP_TRY(h->w_val1.reserve(D));
      PLVS_HIP_TRY(h->heads.reserve(D));
      const int key_bits = voxel_key_bits(chunks);
      const bool ten = key_bits <= 20;   // (two passes of ten bits instead of three of eight)
      const int passes = ten ? 2 : (key_bits + 7) / 8;
      if (ten) launch_sort_medium<10>(h, c.ntiles, passes, guard, q);
      else launch_sort_medium<8>(h, c.ntiles, passes, guard, q);
      skeys = (passes & 1) ? h->dkey1.p : h->dkey0.p;
      sval = (passes & 1) ? h->w_val1.p : h->w_val0.p;
      break;
    }
    case kSortGeneral: {
      int rc = sort_runs(h, D, c.ntiles, chunks, q, &skeys, &sval, guard);
      if (rc != PLVS_OK) return rc;
      PLVS_HIP_TRY(h->heads.reserve(D));
      PLVS_HIP_TRY(h->w_dummy.reserve((size_t)c.max_chunks + 1));
      hipLaunchKernelGGL(voxel_heads, dim3(ceil_div(D, 256 * kHeadTiles)), dim3(256), 0, q, skeys, D, h->heads.p, h->w_dummy.p,
                         h->d_wctr + 1, guard ? (const uint32_t*)&h->d_wctr[1].num_desc : (const uint32_t*)nullptr);
      break;
    }
  }
  return launch_fold(h, c, D, skeys, sval, guard ? (const uint32_t*)guard->skip : (const uint32_t*)nullptr, q);
}

// The runs of a long call whose tiles all went through walk_fast, chunk by chunk (runs_count ... parts_place): behind the
// list of the updated chunks (ev_seg), no pass that sorts all runs.  What it cannot take sets `skip` — the fold then
// leaves at once and the sorting chain runs once the call's counters are read (as for a predicted chain whose bounds
// did not hold).
static int collect_chain(plvs_tsdf_chisel* h, const WalkPlan& plan, const WalkCall& c, uint32_t D, hipStream_t q) {
  const uint32_t rows = plan.collect_rows, blocks = plan.collect_blocks;
  PLVS_HIP_TRY(hipStreamWaitEvent(q, h->ev_seg, 0));
  hipLaunchKernelGGL(runs_scatter, dim3(blocks * (kSegSpan / 256)), dim3(256), 0, q, h->w_seg.p, h->w_rseg.p, c.ntiles, h->w_seg_cnt.p,
                     h->w_active_idx.p, rows, blocks, h->w_run_matrix.p, h->w_rpre.p, h->w_item_base.p, h->d_wctr, h->w_val0.p);
  const unsigned part_grid = (unsigned)std::min<size_t>(plan.parts_cap, 4096);
  hipLaunchKernelGGL(parts_count, dim3(part_grid), dim3(256), 0, q, h->w_part_item.p, h->w_item_part0.p, h->w_item_base.p,
                     h->w_item_cnt.p, h->w_runkey.p, h->d_wctr, h->w_val0.p, h->dkey0.p, h->w_phist.p);
  hipLaunchKernelGGL(rows_heads, dim3(std::min<uint32_t>(ceil_div(rows, 4), 1024u)), dim3(256), 0, q, h->w_item_part0.p,
                     h->w_item_cnt.p, h->w_phist.p, h->d_wctr, rows, h->w_row_heads.p, h->w_row_tot.p);
  hipLaunchKernelGGL(parts_place, dim3(part_grid), dim3(512), 0, q, h->w_part_item.p, h->w_item_part0.p, h->w_item_base.p,
                     h->w_item_cnt.p, h->w_phist.p, h->d_wctr, h->dkey0.p, h->w_val0.p, h->dkey1.p, h->w_val1.p, h->heads.p,
                     h->w_row_heads.p, rows, h->w_row_tot.p);
  return launch_fold(h, c, D, h->dkey1.p, h->w_val1.p, &h->d_wctr[1].skip, q);
}

// The collected chain's buffers, and its run matrix zeroed on the side stream while the walk runs (runs_count writes the
// cells that hold runs, and waits for ev_zero: long over by then).
static int reserve_collect(plvs_tsdf_chisel* h, const WalkPlan& plan, const WalkScratch& w, int max_chunks) {
  const uint32_t rows = plan.collect_rows;
  PLVS_HIP_TRY(h->w_rseg.reserve(h->w_seg.cap));
  PLVS_HIP_TRY(h->w_rpre.reserve(w.seg_own));
  PLVS_HIP_TRY(h->w_active_idx.reserve((size_t)max_chunks));
  PLVS_HIP_TRY(h->w_run_matrix.reserve((size_t)rows * plan.collect_blocks));
  PLVS_HIP_TRY(h->w_item_base.reserve(rows));
  PLVS_HIP_TRY(h->w_item_cnt.reserve(rows));
  PLVS_HIP_TRY(h->w_item_part0.reserve(rows));
  PLVS_HIP_TRY(h->w_row_heads.reserve(rows));
  PLVS_HIP_TRY(h->w_row_tot.reserve((size_t)rows * kSlabVox));
  PLVS_HIP_TRY(h->dkey0.reserve(plan.collect_bound));
  PLVS_HIP_TRY(h->dkey1.reserve(plan.collect_bound));
  PLVS_HIP_TRY(h->w_val0.reserve(plan.collect_bound));
  PLVS_HIP_TRY(h->w_val1.reserve(plan.collect_bound));
  PLVS_HIP_TRY(h->heads.reserve(plan.collect_bound));
  PLVS_HIP_TRY(h->w_part_item.reserve(plan.parts_cap));
  PLVS_HIP_TRY(h->w_phist.reserve(plan.parts_cap * kSlabVox));
  PLVS_HIP_TRY(hipMemsetAsync(h->w_run_matrix.p, 0, (size_t)rows * plan.collect_blocks * sizeof(uint32_t), h->side));
  PLVS_HIP_TRY(hipEventRecord(h->ev_zero, h->side));
  return PLVS_OK;
}

// The call's offsets, tile table, first point and cloud of every tile (the colour fold would otherwise search the cloud
// table once per RUN; the walk's tiles read both instead of searching: tile_span_tables) and, for depth images, the grid
// description, in pinned memory: walk_prologue copies them to the device.  Tiles: 512 consecutive points of one cloud
// (tsdf_directory.hpp), or 32 x 16 blocks of grid pixels.
constexpr size_t kGridWords = (sizeof(GridSrc) + 3) / 4;
static_assert(sizeof(GridSrc) % 4 == 0 && alignof(GridSrc) <= 8, "GridSrc travels as words behind the offsets");
static int fill_call_tables(plvs_tsdf_chisel* h, const int32_t* offsets, int nclouds, const GridSrc* gsrc, uint32_t* ntiles_out,
                            size_t* table_words_out) {
  size_t tiles_of_call = 0;
  for (int c = 0; c < nclouds; ++c) tiles_of_call += ((size_t)(offsets[c + 1] - offsets[c]) + kWalkRays - 1) / kWalkRays;
  const size_t grid_tiles = gsrc ? (size_t)nclouds * gsrc->ntx * gsrc->nty : 0;
  if (gsrc) PLVS_REQUIRE(grid_tiles < 0x7FFFFFFFull, "too many images in one call");
  const size_t table_words = 2 * ((size_t)nclouds + 1) + 2 * tiles_of_call + (gsrc ? kGridWords : 0);
  if (h->h_offsets_cap < table_words) {
    if (h->h_offsets) (void)hipHostFree(h->h_offsets);
    h->h_offsets = nullptr;
    h->h_offsets_cap = 0;
    PLVS_HIP_TRY(hipHostMalloc((void**)&h->h_offsets, (2 * table_words + 64) * sizeof(int32_t)));
    h->h_offsets_cap = 2 * table_words + 64;
  }
  // (depth images: zeros, the table is unused; the walk's copy of the grid description travels behind it)
  const uint32_t cloud_tiles = plvs::tsdf::fill_tile_table(offsets, nclouds, h->h_offsets, kWalkRays);
  const uint32_t ntiles = gsrc ? (uint32_t)grid_tiles : cloud_tiles;
  int32_t* tf = h->h_offsets + 2 * ((size_t)nclouds + 1);
  if (gsrc) memcpy(tf, gsrc, sizeof(GridSrc));
  size_t t = 0;
  for (int c = 0; c < nclouds; ++c)
    for (int32_t p = offsets[c]; p < offsets[c + 1]; p += kWalkRays) {
      tf[ntiles + t] = c;
      tf[t++] = p;
    }
  *ntiles_out = ntiles;
  *table_words_out = table_words;
  return PLVS_OK;
}

// What every attempt of a call of ntiles tiles needs, whatever its plan.
static int reserve_call(plvs_tsdf_chisel* h, uint32_t ntiles, size_t table_words) {
  const size_t max_chunks = (size_t)h->prm.max_chunks;
  PLVS_HIP_TRY(h->offsets.reserve(table_words));
  PLVS_HIP_TRY(h->tile_state.reserve((size_t)ntiles + 1));
  int rc = reserve_chunk_tables(h, max_chunks, std::min<uint32_t>((uint32_t)max_chunks, 64u));
  if (rc != PLVS_OK) return rc;
  PLVS_HIP_TRY(h->w_seg_cnt.reserve(ntiles));
  PLVS_HIP_TRY(h->w_tile_visits.reserve(ntiles));
  PLVS_HIP_TRY(h->w_deferred.reserve(3 * (size_t)ntiles));   // (three lists: one behind each lean pass)
  PLVS_HIP_TRY(h->w_run_cnt.reserve(ntiles));
  PLVS_HIP_TRY(h->dkey0.reserve(kSmallRuns));
  PLVS_HIP_TRY(h->w_val0.reserve(kSmallRuns));
  PLVS_HIP_TRY(h->heads.reserve(kSmallRuns));
  PLVS_HIP_TRY(h->w_run_off.reserve((size_t)ntiles + 1));
  PLVS_HIP_TRY(h->scratch.reserve(scan_scratch_words(ntiles)));
  return PLVS_OK;
}

// The finished call: what the next call's plan takes from it, the developer trace, the stats, the stage times.
static int finish_call(plvs_tsdf_chisel* h, uint32_t ntiles, int chunks_before, const timespec& t0, bool trace) {
  const WalkCounters& c = *h->h_wctr;
  h->num_chunks = h->h_ctr->num_chunks;
  adapt_after_call(h->walk, WalkOutcome{h->h_wctr[1].num_desc, c.ndeferred, c.ndeferred2, c.over_small}, ntiles);
  if (trace) {
    timespec t1;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    fprintf(stderr, "[tsdf_chisel] %.0f us ", (double)(t1.tv_sec - t0.tv_sec) * 1e6 + (double)(t1.tv_nsec - t0.tv_nsec) * 1e-3);
    fprintf(stderr, "[tsdf_chisel] tiles %u deferred %u split %u visits %llu runs %u updated %u parts %u multi %u "
            "rec_top %u seg_top %u voxels %u max_run %u chunks %d chain %d%s\n", ntiles, c.ndeferred * 1000u + c.ndeferred2 + c.ndeferred3 * 1000000u, c.split_tiles,
            (unsigned long long)c.total_visits, h->h_wctr[1].num_desc, c.num_updated, c.num_parts, c.num_multi, c.rec_top,
            c.seg_top, c.num_heads, c.max_run, h->num_chunks, h->last_chain, h->last_chain_skipped ? " REPEATED" : "");
  }
  h->stats.visits = (int64_t)c.total_visits;
  h->stats.new_chunks = h->num_chunks - chunks_before;
  h->stats.updated_chunks = (int32_t)c.num_updated;
  h->stats.voxels = (int32_t)c.num_heads;
  h->stats.max_run = (int32_t)c.max_run;
  h->last_updated = c.num_updated;
  // Part accumulators for the next call: a chunk beyond them is applied in ONE part — never wrong, but on a stream of new
  // views the busy chunks of a call are not those of the call before, and a single 1 500-segment item then is the
  // whole stage (0.4 ms).  Room for twice the chunks this call updated (98 KB each), grown geometrically.
  const uint32_t max_chunks = (uint32_t)h->prm.max_chunks;
  const uint32_t want = std::min<uint32_t>(max_chunks, std::max(c.num_multi + c.num_multi / 2, 2u * c.num_updated));
  if (want > h->multi_cap) {
    int rc = ensure_part_acc(h, std::min<uint32_t>(max_chunks, std::max(want, 2u * h->multi_cap)));
    if (rc != PLVS_OK) return rc;
  }
  if (h->profiling) {
    int rc = add_stage_times(h, 0, kWalkStages);   // (the last one: what the colour fold adds behind the apply stage)
    if (rc != PLVS_OK) return rc;
    h->prof_calls++;
  }
  return PLVS_OK;
}

// gsrc (plvs_hip_tsdf_chisel_integrate_depth_batch_dev): the clouds are depth images — tiles are 32 x 16 blocks of grid
// pixels (GridSrc, tsdf_walk.hpp), d_xyz is null, d_rgb = the colour images, d_kfid = one id per image, offsets =
// nclouds + 1 zeros (nothing reads them).
static int integrate_walk_acc(plvs_tsdf_chisel* h, const float* d_xyz, const uint8_t* d_rgb, const uint32_t* d_kfid,
                              int n, int nclouds, const int32_t* offsets, const float* d_Twc, hipStream_t s,
                              const GridSrc* gsrc = nullptr) {
  // developer switches, read once per process: the collected chain (0 never, 1 long calls, 2 every call — tests); at most
  // this many chunks' rows in its run matrix (tests: calls that update more repeat their chain); a line per call on stderr
  static const int collect_mode = plvs::env_int("PLVS_TSDF_COLLECT", 1, 0, 2);
  static const int max_row_chunks = plvs::env_int("PLVS_TSDF_COLLECT_MAX_ROWS", 0, 0, 1 << 20);
  static const bool trace = plvs::env_int("PLVS_HIP_TSDF_TRACE", 0, 0, 1) != 0;
  const int max_chunks = h->prm.max_chunks;
  uint32_t ntiles = 0;
  size_t table_words = 0;
  int rc = fill_call_tables(h, offsets, nclouds, gsrc, &ntiles, &table_words);
  if (rc != PLVS_OK) return rc;
  if ((size_t)ntiles * kRecStride + (1 << 16) >= 0xFFFFFFFFull) {
    plvs::set_error("tsdf_chisel integrate: %d points in one call exceed the record index range (split the batch)", n);
    return PLVS_ERR_CAPACITY;
  }
  if ((rc = reserve_call(h, ntiles, table_words)) != PLVS_OK) return rc;
  WalkScratch scratch = walk_scratch(h, ntiles);
  h->stage_set = 1;
  const int chunks_before = h->num_chunks;
  timespec trace_t0;   // (developer trace: the call's time on the host's clock)
  clock_gettime(CLOCK_MONOTONIC, &trace_t0);
  uint32_t* const counts[3] = {&h->d_wctr->ndeferred, &h->d_wctr->ndeferred2, &h->d_wctr->ndeferred3};
  uint32_t* const side_ctr = &h->d_wctr[1].num_desc;   // the run count: the scan of the tiles' run counts leaves it there
  for (int attempt = 0;; ++attempt) {
    if ((rc = reserve_walk_scratch(h, ntiles, scratch)) != PLVS_OK) return rc;
    const WalkPlan plan = plan_walk_call(WalkPlanInput{ntiles, attempt, max_chunks, chunks_before, h->run_r1_log2, h->walk,
                                                       h->last_updated, collect_mode, max_row_chunks});
    if (plan.collect_ready && (rc = reserve_collect(h, plan, scratch, max_chunks)) != PLVS_OK) return rc;
    hipLaunchKernelGGL(walk_prologue, dim3(ceil_div((size_t)std::max(max_chunks, nclouds + 1), 256)), dim3(256), 0, s, d_Twc,
                       nclouds, h->poses.p, (const int32_t*)h->h_offsets, h->offsets.p, h->d_wctr, h->d_ctr, h->w_chunk_nseg.p,
                       max_chunks, gsrc ? (int)kGridWords : (int)(2 * ntiles));
    PLVS_HIP_TRY(stage_mark(h, 0, s));
    const WalkCall call{d_xyz, d_rgb, d_kfid, n, nclouds, ntiles, max_chunks, gsrc,
                        gsrc ? reinterpret_cast<const GridSrc*>(h->offsets.p + 2 * ((size_t)nclouds + 1)) : nullptr,
                        scratch.seg_own + scratch.seg_spill, walk_out(h, scratch, h->w_chunk_nseg.p),
                        RunOut{h->w_runkey.p, h->w_masks.p, h->w_run_cnt.p, h->run_r1_log2, plan.collect_ready ? h->w_rseg.p : nullptr},
                        counts[plan.last_list], plan.chain == kChainCollected ? ++h->seq_next : 0u};
    launch_walk_passes(h, plan, call, s);
    if (plan.record_fork) PLVS_HIP_TRY(hipEventRecord(h->ev_fork, s));   // (an event between two kernels of a stream costs ~8 us)
    PLVS_HIP_TRY(stage_mark(h, 1, s));
    // ---- segment sort + apply, and the colour chain the plan names.  (The host issues the critical branch first: a
    // one-key-frame walk is over before a dozen launches have been made.)
    bool collected = false, scanned = false;   // collected: the chain that folded; scanned: w_run_off holds this call's offsets
    if (plan.chain == kChainPredicted) {
      // On the sizes of the call before; a bound that does not hold costs the chain a second time (the fold of the first
      // skips itself).  The chain — a dozen dependent launches, the longer branch — stays on the caller's stream; segment
      // sort and apply go to the side stream and are long over when it ends, or, under the small bound, in front of it.
      if (plan.serial_small && (rc = segments_and_apply(h, plan, call, s)) != PLVS_OK) return rc;
      if ((scanned = plan.scan_first))
        PLVS_HIP_TRY(exclusive_scan_u32(h->w_run_cnt.p, h->w_run_off.p, ntiles, side_ctr, h->scratch.p, s));
      const RunGuard guard{plan.run_bound, side_ctr, &h->d_ctr->num_chunks, plan.chunk_bound, &h->d_wctr[0].err,
                           &h->d_wctr[1].skip, 1u, nullptr, 0u};
      if ((rc = colour_chain(h, call, plan.run_bound, plan.chunk_bound, &guard, s)) != PLVS_OK) return rc;
      if (plan.apply_on_side) {
        PLVS_HIP_TRY(hipStreamWaitEvent(h->side, h->ev_fork, 0));
        if ((rc = segments_and_apply(h, plan, call, h->side)) != PLVS_OK) return rc;
      }
    } else {
      if ((rc = segments_and_apply(h, plan, call, s)) != PLVS_OK) return rc;
      const size_t last_count_word = call.last_count - reinterpret_cast<const uint32_t*>(h->d_wctr);   // (in h_wctr once read)
      if (plan.chain == kChainCollected) {
        // A long call over new ground, not the handle's first: the runs chunk by chunk, queued behind the walk without a
        // read of its counters — the kernels decide themselves whether the call is theirs (runs_count, rows_place: `skip`).
        // The walk's counters are published all the same (rows_place) and read while the chain is queued: when a tile
        // reached walk_tiles or a segment spilled, the chain's kernels leave at once and the sorting chain is queued
        // behind them now, not after the call's last kernel.
        if ((rc = collect_chain(h, plan, call, plan.collect_bound, h->side)) != PLVS_OK) return rc;
        if ((rc = wait_published(h, call.collect_seq, h->side, 1, plan.size_class)) != PLVS_OK) return rc;
        const uint32_t left_to_walk_tiles = reinterpret_cast<const uint32_t*>(h->h_wctr)[last_count_word];
        collected = !(h->h_wctr[0].err == 0 && (left_to_walk_tiles != 0u || h->h_wctr[0].seg_top != 0u));
        if (!collected) {
          scanned = true;
          PLVS_HIP_TRY(exclusive_scan_u32(h->w_run_cnt.p, h->w_run_off.p, ntiles, side_ctr, h->scratch.p, h->side));
          if ((rc = read_walk_counters(h, h->side, plan.size_class, 2)) != PLVS_OK) return rc;   // (kind 2: a short wait of its own expectation)
          const uint32_t D = h->h_wctr[1].num_desc;
          if (D > 0 && (rc = colour_chain(h, call, D, h->h_ctr->num_chunks, nullptr, h->side)) != PLVS_OK) return rc;
        }
      } else {
        // On the call's own counts: the walk is over when they arrive; segment sort and apply are queued behind it.
        PLVS_HIP_TRY(hipStreamWaitEvent(h->side, h->ev_fork, 0));
        scanned = true;
        PLVS_HIP_TRY(exclusive_scan_u32(h->w_run_cnt.p, h->w_run_off.p, ntiles, side_ctr, h->scratch.p, h->side));
        if ((rc = read_walk_counters(h, h->side, plan.size_class, 1)) != PLVS_OK) return rc;
        const uint32_t D = h->h_wctr[1].num_desc;
        collected = collect_on_own_counts(plan, reinterpret_cast<const uint32_t*>(h->h_wctr)[last_count_word], h->h_wctr[0].seg_top, D);
        if (h->h_wctr[0].err == 0 && D > 0) {
          rc = collected ? collect_chain(h, plan, call, D, h->side) : colour_chain(h, call, D, h->h_ctr->num_chunks, nullptr, h->side);
          if (rc != PLVS_OK) return rc;
        }
      }
    }
    if (!plan.serial_small) {   // (the side stream had a branch)
      PLVS_HIP_TRY(hipEventRecord(h->ev_join, h->side));
      PLVS_HIP_TRY(hipStreamWaitEvent(s, h->ev_join, 0));
    }
    PLVS_HIP_TRY(stage_mark(h, 4, s));
    if ((rc = read_walk_counters(h, s, plan.size_class)) != PLVS_OK) return rc;
    const uint32_t err = h->h_wctr->err;
    if (err & ~kErrScratch) return walk_fail(h, err);
    if (err & kErrScratch) {   // the map is untouched (apply_chunks left at once, no colours folded): grow and repeat
      if (attempt >= 8 || !grow_walk_scratch(h, ntiles, scratch)) return walk_fail(h, err);
      continue;
    }
    h->last_chain = collected ? kChainCollected : plan.chain == kChainPredicted ? kChainPredicted : kChainOwn;
    h->last_chain_skipped = h->last_chain != kChainOwn && h->h_wctr[1].skip != 0u;
    if (h->last_chain_skipped) {   // the bounds did not hold: the chain once more, with the call's numbers
      if (!scanned) PLVS_HIP_TRY(exclusive_scan_u32(h->w_run_cnt.p, h->w_run_off.p, ntiles, side_ctr, h->scratch.p, s));
      PLVS_HIP_TRY(hipMemsetAsync(&h->d_wctr[1].num_heads, 0, sizeof(uint32_t), s));
      PLVS_HIP_TRY(hipMemsetAsync(&h->d_wctr[1].num_updated, 0, sizeof(uint32_t), s));
      if ((rc = colour_chain(h, call, h->h_wctr[1].num_desc, h->h_ctr->num_chunks, nullptr, s)) != PLVS_OK) return rc;
      if ((rc = read_walk_counters(h, s, plan.size_class)) != PLVS_OK) return rc;
    }
    break;
  }
  return finish_call(h, ntiles, chunks_before, trace_t0, trace);
}
