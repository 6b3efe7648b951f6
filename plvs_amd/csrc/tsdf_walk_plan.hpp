// The policy of the order-free chisel integrate (integrate_walk_acc, tsdf_chisel_order_free.hpp): every decision of one attempt of a
// call as data, made from the call's size and what the handle remembers of the call before.  Plain C++17, no HIP: the
// driver launches what the plan says, tests/host/walk_plan_host.cpp compiles this header with a host compiler.
// The measurements behind the thresholds: DESIGN §4.1-4.5.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace plvs {
namespace tsdf {

constexpr uint32_t kSmallCallTiles = 320;     // a few key frames: one tile per CU is all there is to run
constexpr uint32_t kPredictTiles = 4096;      // calls up to this size (~25 key frames) launch their colour chain on the sizes of the call before
constexpr uint32_t kSortSmallRuns = 4096;     // runs the one-launch sort takes (sort_runs_small; = kSmallRuns, tsdf_walk.hpp)
constexpr uint32_t kSortMediumRuns = 16384;   // ... and the one-workgroup sort (sort_runs_medium) ...
constexpr uint32_t kSortMediumTiles = 2048;   // ... of a call of few tiles: it lists the runs in one workgroup's loop over the tiles
constexpr size_t kPredictRuns = 200000;       // a long call expecting at most this many runs is predicted (collect mode 0 only)
constexpr uint32_t kCollectMinRuns = 65536;   // fewer runs do not pay the collected chain's launches
constexpr uint32_t kCollectPartRuns = 4096;   // (= kCollectPart)
constexpr uint32_t kRowsPerChunk = 8;         // (= kSlabs)
constexpr uint32_t kTileSegments = 64;        // (= kWalkChunks)
constexpr uint32_t kSegmentBlock = 1024;      // (= kSegSpan)

// How D runs of a call of ntiles tiles are sorted.  Only the general chain (compact_runs + radix sort) reads the scanned
// run counts; the other two sum the tiles' counts themselves.
enum SortKind { kSortSmall = 0, kSortMedium = 1, kSortGeneral = 2 };
inline SortKind sort_kind(uint32_t D, uint32_t ntiles) {
  if (D <= kSortSmallRuns) return kSortSmall;
  return (ntiles <= kSortMediumTiles && D <= kSortMediumRuns) ? kSortMedium : kSortGeneral;
}
inline bool sort_needs_scan(uint32_t D, uint32_t ntiles) { return sort_kind(D, ntiles) == kSortGeneral; }

struct WalkHistory {   // what the handle keeps from the call before
  bool small_runs_known = false;   // the two below are a call's
  uint32_t small_runs_last = 0, small_tiles_last = 1;
  bool walk_small = false;         // first lean pass with 1024 entries instead of 2048
  bool third_pass = false;         // a 4096-entry pass behind the 1024- and the 2048-entry one
};

struct WalkPlanInput {
  uint32_t ntiles = 0;
  int attempt = 0;
  int max_chunks = 0, chunks_before = 0;
  uint32_t run_r1_log2 = 11;   // run slots per tile (log2)
  WalkHistory hist;
  uint32_t last_updated = 0;   // chunks the handle's last call (of any kind) updated
  int collect_mode = 1;        // 0 never / 1 long calls / 2 every call
  int max_row_chunks = 0;      // 0: no cap on the chunks of the run matrix
};

// The colour chain of an attempt, as the trace prints it: on the call's own counts (behind a read of the walk's counters),
// on the sizes of the call before, or collected chunk by chunk and queued without a read.
enum ChainKind { kChainOwn = 0, kChainPredicted = 1, kChainCollected = 2 };

struct WalkPass {    // one lean pass (walk_fast)
  int entries;       // table size: 1024, 2048 or 4096
  uint32_t grid;     // workgroups
  int src, dst;      // deferred lists 0..2 it reads (-1: every tile) and writes
};

struct WalkPlan {
  int size_class = 0;          // 0: a few key frames, 1: tens, 2: a hundred
  int npasses = 0;
  WalkPass pass[3] = {};
  int last_list = 0;           // walk_tiles walks this list ...
  uint32_t pieces = 2;         // ... in this many pieces per tile (what overflowed a 2048-entry table goes whole)
  ChainKind chain = kChainOwn;
  bool collect_ready = false;  // the collected chain's buffers are reserved: kChainCollected, or kChainOwn that may turn to it
  bool collect_any_count = false;   //   ... whatever the number of runs (collect mode 2)
  bool serial_small = false;   // predicted on the small bound: everything on the caller's stream
  bool apply_on_side = false;  // predicted: segment sort + apply on the side stream, the chain on the caller's (every other chain: the reverse)
  bool record_fork = true;     // an event behind the walk for the other stream
  bool scan_first = false;     // predicted: the run counts are scanned in front of the chain
  uint32_t run_bound = 0;      // predicted: the chain's bounds
  int chunk_bound = 0;
  uint32_t collect_rows = 0, collect_blocks = 0, collect_bound = 0;   // the run matrix and the most runs the chain's buffers hold
  size_t parts_cap = 0;
};

inline WalkPlan plan_walk_call(const WalkPlanInput& in) {
  const uint32_t T = in.ntiles;
  const WalkHistory& hs = in.hist;
  const int M = in.collect_mode;
  WalkPlan p;
  p.size_class = T <= kSmallCallTiles ? 0 : (T <= kPredictTiles ? 1 : 2);

  // ---- the walk: a tile alone in a lean kernel; what overflows its table goes to the next larger one, then to walk_tiles
  if (T <= kSmallCallTiles) {
    p.pass[p.npasses++] = WalkPass{4096, T, -1, 0};
  } else {
    // the first pass's table follows the scene (adapt_after_call): tiles of near surfaces fit 1024 entries, three to a CU
    p.pass[p.npasses++] = WalkPass{hs.walk_small ? 1024 : 2048, T, -1, 0};
    if (hs.walk_small) {
      p.pass[p.npasses++] = WalkPass{2048, std::min<uint32_t>(T, 1024u), 0, 1};
      // (a launch that finds an empty list costs the stream 8 us: only when the call before had such tiles)
      if (hs.third_pass) p.pass[p.npasses++] = WalkPass{4096, std::min<uint32_t>(T, 512u), 1, 2};
    } else {
      p.pass[p.npasses++] = WalkPass{4096, std::min<uint32_t>(T, 512u), 0, 1};
    }
  }
  p.last_list = p.pass[p.npasses - 1].dst;
  p.pieces = p.pass[p.npasses - 1].entries == 2048 ? 1u : 2u;

  // ---- the colour chain
  const double tiles_last = (double)std::max(1u, hs.small_tiles_last);
  const size_t E = hs.small_runs_known ? (size_t)((double)hs.small_runs_last * (double)T / tiles_last) : ~(size_t)0;
  // A call of up to kPredictTiles tiles launches its chain on the sizes of the call before instead of waiting for its own;
  // so does a long call once the map has saturated, unless the collected chain takes it (queued without the counts as well).
  const bool predicted = hs.small_runs_known && in.attempt == 0 && M != 2 && (T <= kPredictTiles || (E <= kPredictRuns && M == 0));
  p.collect_ready = M != 0 && (T > kPredictTiles || M == 2) && !predicted;
  p.collect_any_count = M == 2;
  const bool collect_queued = p.collect_ready && hs.small_runs_known && in.attempt == 0;
  p.chain = predicted ? kChainPredicted : (collect_queued ? kChainCollected : kChainOwn);
  // (the small bound is ONE sorting launch: a branch on another stream starts ~20 us after the event it waits for and is
  // joined ~20 us after it ends — more than the chain itself)
  p.serial_small = predicted && E <= kSortSmallRuns / 2;
  p.apply_on_side = predicted && !p.serial_small;
  p.record_fork = !collect_queued;   // (nothing for the side stream before the counting stages are over: ev_seg)
  if (predicted) {
    const size_t slots = (size_t)T << in.run_r1_log2;
    // (the call before scaled to this call's tiles, a quarter more, padded to the sort's tiles)
    p.run_bound = E <= kSortSmallRuns / 2 ? kSortSmallRuns : (uint32_t)std::min<size_t>(slots, (E * 5 / 4 + 8191) / 4096 * 4096);
    // (a moderate expectation: the one-workgroup sort on its full capacity — a bound that costs nothing)
    if (T <= kSortMediumTiles && p.run_bound > kSortSmallRuns && E * 5 / 4 + 1024 <= kSortMediumRuns) p.run_bound = kSortMediumRuns;
    p.chunk_bound = std::min(in.max_chunks, std::max(2 * in.chunks_before, in.chunks_before + 256));
    p.scan_first = sort_needs_scan(p.run_bound, T);
  }

  // ---- the collected chain's geometry: (chunk, slab) rows for twice the chunks the call before updated — a power of two,
  // so that the matrix is re-allocated when a stream's calls update twice the chunks, not a few more each time
  size_t row_chunks = 256;
  while (row_chunks < 2 * (size_t)in.last_updated + 64) row_chunks *= 2;
  if (in.max_row_chunks > 0) row_chunks = std::min<size_t>(row_chunks, (size_t)in.max_row_chunks);
  p.collect_rows = (uint32_t)std::min<size_t>((size_t)in.max_chunks, row_chunks) * kRowsPerChunk;
  p.collect_blocks = (uint32_t)(((size_t)T * kTileSegments + kSegmentBlock - 1) / kSegmentBlock);
  // (four times the call before scaled to this call's tiles, 8 M at least, never more than the tiles' run slots)
  p.collect_bound = (uint32_t)std::min<size_t>(
      (size_t)T << in.run_r1_log2,
      std::max<size_t>((size_t)8 << 20, hs.small_runs_known ? (size_t)(4.0 * (double)hs.small_runs_last * (double)T / tiles_last) : 0));
  p.parts_cap = (size_t)p.collect_bound / kCollectPartRuns + p.collect_rows + 1;
  return p;
}

// A chain on the call's own counts: collected when no tile was left to walk_tiles (its runs are not grouped by chunk), no
// segment spilled and the runs pay the chain's launches.
inline bool collect_on_own_counts(const WalkPlan& p, uint32_t left_to_walk_tiles, uint32_t seg_top, uint32_t D) {
  return p.collect_ready && left_to_walk_tiles == 0u && seg_top == 0u && (D > kCollectMinRuns || p.collect_any_count);
}

struct WalkOutcome {   // a finished call's counters, as far as the next call's plan depends on them
  uint32_t runs = 0;
  uint32_t ndeferred = 0, ndeferred2 = 0;   // tiles the first / the second lean pass deferred
  uint32_t over_small = 0;                  // tiles of a 2048-entry first pass that a 1024-entry table would not have held
};

inline void adapt_after_call(WalkHistory& hs, const WalkOutcome& c, uint32_t ntiles) {
  if (ntiles > kSmallCallTiles) {   // the first pass's table for the next call
    if (hs.walk_small) {            // (this call's first pass had 1024 entries)
      hs.third_pass = c.ndeferred2 != 0u;                               // tiles overflowed the 2048-entry table too
      if ((size_t)c.ndeferred * 4 > ntiles) hs.walk_small = false;      // more than a quarter of the tiles overflowed the small table
    } else if ((size_t)c.over_small * 6 <= ntiles) {
      hs.walk_small = true;                                             // at most a sixth would
    }
  }
  hs.small_runs_known = true;   // (the runs of the last call, whatever its length)
  hs.small_runs_last = c.runs;
  hs.small_tiles_last = ntiles;
}

}  // namespace tsdf
}  // namespace plvs
