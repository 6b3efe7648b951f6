// Host compile of the order-free integrate's policy (plvs_amd/csrc/tsdf_walk_plan.hpp): plans, the sort of a run count
// and the feedback after a call as flat arrays of integers.  Test infrastructure only.
#include <cstdint>

#include "../../plvs_amd/csrc/tsdf_walk_plan.hpp"

using namespace plvs::tsdf;

// in: ntiles, attempt, max_chunks, chunks_before, run_r1_log2, small_runs_known, small_runs_last, small_tiles_last,
//     last_updated, walk_small, third_pass, collect_mode, max_row_chunks
static WalkPlan plan_of(const int64_t* in) {
  WalkPlanInput i;
  i.ntiles = (uint32_t)in[0];
  i.attempt = (int)in[1];
  i.max_chunks = (int)in[2];
  i.chunks_before = (int)in[3];
  i.run_r1_log2 = (uint32_t)in[4];
  i.hist.small_runs_known = in[5] != 0;
  i.hist.small_runs_last = (uint32_t)in[6];
  i.hist.small_tiles_last = (uint32_t)in[7];
  i.last_updated = (uint32_t)in[8];
  i.hist.walk_small = in[9] != 0;
  i.hist.third_pass = in[10] != 0;
  i.collect_mode = (int)in[11];
  i.max_row_chunks = (int)in[12];
  return plan_walk_call(i);
}

// out[29]: size_class, npasses, 3 x (entries, grid, src, dst), last_list, pieces, chain, collect_ready, collect_any_count,
//          serial_small, apply_on_side, record_fork, scan_first, run_bound,
//          chunk_bound, collect_rows, collect_blocks, collect_bound, parts_cap
extern "C" void hostplan_plan(const int64_t* in, int64_t* out) {
  const WalkPlan p = plan_of(in);
  int k = 0;
  out[k++] = p.size_class;
  out[k++] = p.npasses;
  for (int i = 0; i < 3; ++i) {
    const bool used = i < p.npasses;
    out[k++] = used ? p.pass[i].entries : 0;
    out[k++] = used ? (int64_t)p.pass[i].grid : 0;
    out[k++] = used ? p.pass[i].src : 0;
    out[k++] = used ? p.pass[i].dst : 0;
  }
  out[k++] = p.last_list;
  out[k++] = p.pieces;
  out[k++] = (int64_t)p.chain;
  out[k++] = p.collect_ready;
  out[k++] = p.collect_any_count;
  out[k++] = p.serial_small;
  out[k++] = p.apply_on_side;
  out[k++] = p.record_fork;
  out[k++] = p.scan_first;
  out[k++] = p.run_bound;
  out[k++] = p.chunk_bound;
  out[k++] = p.collect_rows;
  out[k++] = p.collect_blocks;
  out[k++] = p.collect_bound;
  out[k++] = (int64_t)p.parts_cap;
}

extern "C" int hostplan_sort_kind(uint32_t D, uint32_t ntiles) { return (int)sort_kind(D, ntiles); }
extern "C" int hostplan_sort_needs_scan(uint32_t D, uint32_t ntiles) { return sort_needs_scan(D, ntiles) ? 1 : 0; }

extern "C" int hostplan_collect_on_own_counts(const int64_t* in, uint32_t left_to_walk_tiles, uint32_t seg_top, uint32_t D) {
  return collect_on_own_counts(plan_of(in), left_to_walk_tiles, seg_top, D) ? 1 : 0;
}

// hist (in / out): small_runs_known, small_runs_last, small_tiles_last, walk_small, third_pass
// outcome: runs, ndeferred, ndeferred2, over_small
extern "C" void hostplan_adapt(int64_t* hist, const int64_t* outcome, uint32_t ntiles) {
  WalkHistory h;
  h.small_runs_known = hist[0] != 0;
  h.small_runs_last = (uint32_t)hist[1];
  h.small_tiles_last = (uint32_t)hist[2];
  h.walk_small = hist[3] != 0;
  h.third_pass = hist[4] != 0;
  WalkOutcome c;
  c.runs = (uint32_t)outcome[0];
  c.ndeferred = (uint32_t)outcome[1];
  c.ndeferred2 = (uint32_t)outcome[2];
  c.over_small = (uint32_t)outcome[3];
  adapt_after_call(h, c, ntiles);
  hist[0] = h.small_runs_known;
  hist[1] = h.small_runs_last;
  hist[2] = h.small_tiles_last;
  hist[3] = h.walk_small;
  hist[4] = h.third_pass;
}
