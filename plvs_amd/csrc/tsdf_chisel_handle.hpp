// The map handle of the open_chisel back end and what every pipeline that works on it shares: the per-call counters and
// the kernels that publish them, the reads of those counters, the stage times, the failure paths.  tsdf_chisel.hip and the
// tsdf_chisel_*.hpp headers of its pipelines (one translation unit) include it.
#pragma once
#include <vector>

#include "common.hpp"
#include "device_utils.hpp"
#include "tsdf_chisel_core.hpp"
#include "tsdf_directory.hpp"
#include "tsdf_chisel_view.hpp"
#include "tsdf_walk.hpp"
#include "tsdf_walk_plan.hpp"

using namespace plvs;   // (a private header of one translation unit)
using namespace plvs::chisel;
using namespace plvs::tsdf;

namespace {

// Stage names of the ordered pipeline (tsdf_chisel_ordered.hpp) and of the order-free / ray-sharded ones
// (tsdf_chisel_order_free.hpp, tsdf_chisel_shard.hpp); plvs_tsdf_chisel::stage_set says which the times belong to.
constexpr int kNumStages = 6;
const char* const kStageNames[kNumStages] = {"ray_count", "scan", "ray_tiles", "sort_runs",
                                             "gather_runs", "chain_runs"};
constexpr int kWalkStages = 4;
const char* const kWalkStageNames[kWalkStages] = {"walk_tiles", "sort_segments", "apply_chunks", "fold_colours"};

struct Counters {           // device-side, read back once per call
  uint32_t total_visits;
  int32_t num_chunks;
  uint32_t err;
  uint32_t num_heads;
  uint32_t num_updated;
  uint32_t max_run;
  uint32_t num_desc;
};

__global__ void pose_prep(const float* __restrict__ Twc, int nclouds, Pose* __restrict__ poses) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nclouds) make_pose(Twc + 12 * c, &poses[c]);
}

// Counters -> their pinned host copies by a kernel's stores: a small device-to-host copy command costs tens of
// microseconds of queueing, a store through the host-mapped pointer a few.
// host_seq (the order-free pipeline's reads): after the counters a sequence number, stored with system scope — the host polls that
// word in pinned memory instead of sleeping on the stream (wait_published: a wake-up is 20-30 us, on the critical path of a
// long call's colour chain and a fifth of a one-key-frame call)
__global__ void publish_counters(const WalkCounters* __restrict__ wctr, const Counters* __restrict__ ctr,
                                 WalkCounters* __restrict__ host_wctr, Counters* __restrict__ host_ctr,
                                 uint32_t* __restrict__ host_seq = nullptr, uint32_t seq = 0u) {
  if (wctr) {
    const uint32_t* a = reinterpret_cast<const uint32_t*>(wctr);
    uint32_t* b = reinterpret_cast<uint32_t*>(host_wctr);
    for (int k = threadIdx.x; k < (int)(2 * sizeof(WalkCounters) / sizeof(uint32_t)); k += blockDim.x) b[k] = a[k];
  }
  if (ctr) {
    const uint32_t* c = reinterpret_cast<const uint32_t*>(ctr);
    uint32_t* d = reinterpret_cast<uint32_t*>(host_ctr);
    for (int k = threadIdx.x; k < (int)(sizeof(Counters) / sizeof(uint32_t)); k += blockDim.x) d[k] = c[k];
  }
  __threadfence_system();
  if (host_seq != nullptr) {
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(host_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ... and any few words the same way (up to three ranges per launch).
__global__ void publish_words(const uint32_t* __restrict__ a, uint32_t* __restrict__ ha, int na, const uint32_t* __restrict__ b,
                              uint32_t* __restrict__ hb, int nb, const uint32_t* __restrict__ c, uint32_t* __restrict__ hc, int nc) {
  for (int k = threadIdx.x; k < na; k += blockDim.x) ha[k] = a[k];
  for (int k = threadIdx.x; k < nb; k += blockDim.x) hb[k] = b[k];
  for (int k = threadIdx.x; k < nc; k += blockDim.x) hc[k] = c[k];
  __threadfence_system();
}

}  // namespace

struct ChiselDeformState;   // tsdf_chisel_deform.hpp

struct plvs_tsdf_chisel {
  plvs_tsdf_chisel_params prm;
  Params P;
  Directory dir;
  float* sdf = nullptr;
  float* weight = nullptr;
  uint32_t* kfid = nullptr;
  uint32_t* rgbw = nullptr;
  Counters* d_ctr = nullptr;
  Counters* h_ctr = nullptr;  // pinned
  int num_chunks = 0;         // host mirror
  bool poisoned = false;
  // per-call scratch
  DevBuf<uint32_t> counts, heads, updated, scratch;
  DevBuf<float2> rec, rec_t;         // operands in voxel order / grouped per tile
  DevBuf<uint32_t> recc_t;           // colours, grouped per tile (folded through the sorted runs)
  DevBuf<uint32_t> dkey0, dkey1, run_cnt, run_dst, last_pt;   // run descriptors
  DevBuf<unsigned long long> didx0, didx1;
  DevBuf<uint32_t> tile_first, block_first;
  DevBuf<unsigned long long> tile_state;   // [0]: ticket, [1..]: look-back state per tile
  DevBuf<Pose> poses;
  ChiselDeformState* dfm = nullptr;    // Chisel::Deform: the reference's chunk-map order, kept once enable_deform is on
  void* ext = nullptr;                 // see ChiselMapView::ext
  void (*ext_free)(void*) = nullptr;
  // halo of a sharded map (meshing): ghost copies of other ranks' chunks in the pool slots past num_chunks
  Directory gdir{};                    // id -> ghost slot / kGhostAbsent (allocated by the first import)
  int ghost_count = 0;                 // ghost chunks (pool slots taken) since the last halo_clear
  long long ghost_entries = 0;         //   and directory entries ("absent" answers included)
  DevBuf<uint32_t> halo_row;           // payload row of each request (prefix of the found flags)
  unsigned long long* miss_keys = nullptr;   // the chunks the last meshing pass looked for and did not have
  int32_t* miss_ids = nullptr;
  uint32_t* miss_count = nullptr;
  uint32_t miss_cap = 0, miss_mask = 0;
  DevBuf<int32_t> offsets;
  // host-flavour staging
  DevBuf<float> st_xyz, st_Twc, st_nrm;
  DevBuf<uint8_t> st_rgb;
  DevBuf<uint32_t> st_kfid;
  DevBuf<uint32_t> st_pos, st_scan, st_off;   // depth-image entry of an ordered / sharded / deforming handle: the clouds' scan
  plvs_tsdf_stats stats{};
  uint32_t last_updated = 0;
  // queued key-frame clouds (plvs_hip_tsdf_chisel_queue / _flush): uploaded, not yet integrated
  DevBuf<float> q_xyz;
  DevBuf<uint8_t> q_rgb;
  DevBuf<uint32_t> q_kfid;
  std::vector<int32_t> q_offsets;   // [clouds + 1] once anything is queued
  std::vector<float> q_Twc;         // 12 per cloud
  bool q_kfid_given = false;
  // single-walk pipeline (tsdf_walk.hpp)
  WalkCounters* d_wctr = nullptr;   // [2]: the call's counters, the colour pass's voxel list
  WalkCounters* h_wctr = nullptr;   // pinned
  uint32_t* h_seq = nullptr;        // pinned, coherent: the sequence number of the last publish_counters that has landed
  uint32_t seq_next = 0;
  double wait_ema_us[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};       // how long the host's last waits for the published counters took (wait_published)
  DevBuf<uint4> w_rec, w_seg, w_sorted_seg;
  DevBuf<uint32_t> w_seg_ticket;   // per segment descriptor slot of w_seg: its index among its chunk's segments (AccOut::seg_ticket)
  // a long call's runs chunk by chunk (runs_count ... parts_place): the segments' run descriptors and the runs of the
  // same row in the block's earlier tiles; runs per (row, block); chunk slot -> place among the updated; region, runs and
  // first part of every row; the parts' rows and histograms
  DevBuf<uint4> w_rseg, w_rpre;
  DevBuf<uint32_t> w_run_matrix, w_active_idx, w_item_base, w_item_cnt, w_item_part0, w_part_item, w_phist, w_row_heads, w_row_tot;
  hipEvent_t ev_zero = nullptr;  // the run matrix is zero (side stream -> caller's stream)
  hipEvent_t ev_seg = nullptr;   // the updated chunks are listed (seg_scan; caller's stream -> side stream)
  int last_chain = 0;            // (developer trace) the last call's colour chain: 0 on its own counts, 1 predicted, 2 collected
  bool last_chain_skipped = false;   //   ... and whether it had to be repeated
  DevBuf<uint32_t> w_chunk_nseg, w_chunk_off, w_chunk_fill, w_active_off, w_masks, w_dummy, w_seg_cnt, w_tile_visits, w_deferred;
  DevBuf<uint32_t> w_part_off, w_multi_idx;          // apply stage: parts of the updated chunks
  DevBuf<long long> pa_wuu;                          //   accumulators of the chunks applied in parts (zero between calls)
  DevBuf<unsigned long long> pa_w;
  DevBuf<uint32_t> pa_last, pa_cnt, pa_done;
  uint32_t multi_cap = 0;
  uint32_t part_segs = kPartSegs, part_min = kPartMin;   // (plvs_hip_tsdf_chisel_set_apply_parts)
  plvs::tsdf::WalkHistory walk;   // what the next order-free call's plan takes from the call before (tsdf_walk_plan.hpp)
  DevBuf<uint32_t> w_runkey, w_run_cnt, w_run_off, w_val0, w_val1;   // runs: per-tile regions of 2^run_r1_log2 slots
  int32_t* h_offsets = nullptr;      // pinned copy of the call's cloud offsets
  size_t h_offsets_cap = 0;
  // run slots per tile (log2): 2048 from the start — a tile of the 2048-entry walk can need 1792, and growing the regions
  // later means repeating a call and re-allocating its largest buffers (ntiles << r1_log2 masks of 64 B) in the middle of
  // a job; a tile of the 4096-entry walk that needs more still grows them once
  uint32_t run_r1_log2 = 11;
  float scale_u = 1.f, scale_w = 1.f;   // fixed-point scales of the order-free accumulators (powers of two)
  int stage_set = 0;                    // which pipeline the stage times belong to
  // ray-sharded multi-GPU integrate (tsdf_shard.hpp)
  Directory xdir{};                  // the walk directory: every chunk the rank's tiles have crossed (ids only)
  int32_t* d_xcount = nullptr;
  uint32_t* x_sat = nullptr;         //   + one bit per voxel: its owner has reported the colour saturated
  DevBuf<uint32_t> sh_ctl;
  uint32_t* h_sh_ctl = nullptr;      // pinned [320]
  uint32_t* h_sh_off = nullptr;      // pinned [128 + 132]: region offsets on their way to the device (pack | apply)
  DevBuf<uint4> sh_seg_reg, sh_rec_reg;
  DevBuf<uint32_t> sh_nrec, sh_owner, sh_slot_owner, sh_src_off, sh_run_ctr, sh_vkey, sh_sat;
  DevBuf<uint4> sh_run_first;   // per run of a sharded walk: the first wire record's spans + its number of records
  uint32_t sh_nt = 0, sh_runs = 0, sh_nsat = 0;
  DevBuf<int32_t> sh_wait;   // saturated voxels not yet announced ({chunk x, y, z, voxel}): [sh_wait_first, + sh_wait_count)
  uint32_t sh_wait_first = 0, sh_wait_count = 0;
  long long* h_sh_counts = nullptr;  // pinned
  int sh_n = 0, sh_nclouds = 0;      // the call in flight (shard_walk -> shard_pack -> shard_apply)
  uint32_t sh_ntiles = 0;            // tiles of the whole point stream
  std::vector<int32_t> sh_tiletab;   // the call's offsets + tile table (host copy)
  int sh_phase = 0;
  plvs_tsdf_stats sh_stats{};
  hipStream_t side = nullptr;   // second stream for the colour chain
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // optional per-stage timing (HIP events on the caller's stream)
  bool profiling = false;
  hipEvent_t ev[kNumStages + 1] = {};
  double stage_ms[kNumStages] = {};
  int64_t prof_calls = 0;
};

// Every entry point that reads or changes the map integrates the queued key-frame clouds first (plvs_hip_tsdf_chisel_queue).
extern "C" int plvs_hip_tsdf_chisel_flush(plvs_tsdf_chisel* h);
#define PLVS_FLUSH_QUEUE(h)                                        \
  do {                                                             \
    if ((h) && !(h)->q_offsets.empty()) {                          \
      const int rc_flush_ = plvs_hip_tsdf_chisel_flush(h);         \
      if (rc_flush_ != PLVS_OK) return rc_flush_;                  \
    }                                                              \
  } while (0)

// ---- the reads of the counters

// The ordered pipeline's read (and carving's, the scan integrate's): publish, then sleep on the stream.
static int read_counters(plvs_tsdf_chisel* h, hipStream_t s) {
  hipLaunchKernelGGL(publish_counters, dim3(1), dim3(64), 0, s, (const WalkCounters*)nullptr, h->d_ctr, (WalkCounters*)nullptr,
                     h->h_ctr);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(hipStreamSynchronize(s));
  return PLVS_OK;
}

static inline void cpu_relax() {   // (inside a polling loop)
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__) || defined(__arm__)
  __asm__ __volatile__("yield");
#endif
}

// The host's wait for a publish_counters launch that carried sequence number `seq` on stream q: it polls the word that launch
// stores last, then sleeps on the stream.  Everything enqueued on q before that launch has completed when the word arrives
// (stream order), so this stands for hipStreamSynchronize(q) as far as the pipeline's own buffers and the caller's inputs
// are concerned.
// The host's cost: the calling thread SLEEPS through most of the wait it expects (the handle remembers how long its last waits
// of this kind took: a 100-key-frame step's last wait is ~0.9 ms, a one-key-frame call's ~0.1 ms) and polls only for the
// rest — at most PLVS_TSDF_SPIN_US microseconds (default 400; 0: never poll) before it falls back to hipStreamSynchronize —
// so a SLAM thread next to it loses a core for a few hundred microseconds per call at worst, not for the length of the call.
// kind: 0 the end of a call, 1 the read in front of its colour chain; size_class: calls of a few key frames, of tens, of a hundred
// (their waits differ by an order of magnitude, and a SLAM system alternates them)
static int wait_published(plvs_tsdf_chisel* h, uint32_t seq, hipStream_t q, int kind = 0, int size_class = 0) {
  double& ema = h->wait_ema_us[kind][size_class];
  static const int spin_us = plvs::env_int("PLVS_TSDF_SPIN_US", 400, 0, 10000000);
  if (spin_us > 0 && h->h_seq != nullptr) {
    const volatile uint32_t* const word = h->h_seq;
    timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    auto elapsed_us = [&]() {
      clock_gettime(CLOCK_MONOTONIC, &t1);
      return (double)(t1.tv_sec - t0.tv_sec) * 1e6 + (double)(t1.tv_nsec - t0.tv_nsec) * 1e-3;
    };
    bool done = *word == seq;
    if (!done && ema > 200.0) {   // most of an expected long wait is slept, not polled (timer slack: ~60 us)
      timespec nap;
      // (... of a wait of a whole long call — a chain queued without a read of the walk's counters — 70 %: its length follows
      // the view, +-20 % from call to call, and a nap that overshoots is paid in full)
      const double us = std::min(std::min(ema - 120.0, 0.7 * ema), 5000.0);
      nap.tv_sec = 0;
      nap.tv_nsec = (long)(us * 1e3);
      nanosleep(&nap, nullptr);
      done = *word == seq;
    }
    const double spin_from = done ? 0.0 : elapsed_us();
    for (uint32_t spins = 0; !done; ++spins) {
      done = *word == seq;
      if (done) break;
      cpu_relax();
      if ((spins & 255u) == 255u && elapsed_us() - spin_from > (double)spin_us) break;
    }
    if (done) {
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
      ema = 0.75 * ema + 0.25 * elapsed_us();
      return PLVS_OK;
    }
    ema = 0.75 * ema + 0.25 * (elapsed_us() + 200.0);   // (longer than expected: sleep longer next time)
  }
  // (the runtime has not observed the stream's completion after a polled read; nothing below relies on it: buffers are
  // re-used in stream order, and hipFree — DevBuf::reserve — synchronises the device itself)
  PLVS_HIP_TRY(hipStreamSynchronize(q));
  return PLVS_OK;
}

// Both counter blocks, published under a new sequence number and waited for.
static int read_walk_counters(plvs_tsdf_chisel* h, hipStream_t s, int size_class = 0, int kind = 0) {
  const uint32_t seq = ++h->seq_next;
  hipLaunchKernelGGL(publish_counters, dim3(1), dim3(64), 0, s, h->d_wctr, h->d_ctr, h->h_wctr, h->h_ctr, h->h_seq, seq);
  PLVS_KERNEL_CHECK();
  return wait_published(h, seq, s, kind, size_class);
}

// ---- failure: a call that ends with the map in an unknown state poisons the handle (clear() revives it) and reports
// through plvs::set_error

static int poisoned(plvs_tsdf_chisel* h) {   // (behind the call's plvs::set_error)
  h->poisoned = true;
  return PLVS_ERR_CAPACITY;
}

static int walk_fail(plvs_tsdf_chisel* h, uint32_t err) {
  plvs::set_error("tsdf_chisel integrate: %s%s(err=%u)", (err & kErrPoolFull) ? "chunk pool full (raise max_chunks) " : "",
                  (err & kErrCoordRange) ? "voxel coordinates beyond +-2^20 (outside the supported map extent) " : "", err);
  return poisoned(h);
}

// ---- stage times (plvs_hip_tsdf_chisel_set_profiling): event i in front of stage i, on the stream the stage runs on, and
// one more behind the last stage

static hipError_t stage_mark(plvs_tsdf_chisel* h, int i, hipStream_t q) {
  return h->profiling ? hipEventRecord(h->ev[i], q) : hipSuccess;
}

// Time between two stage events of a call the host has read the counters of.  The read polls a word the call's last kernel
// stores to pinned memory (wait_published) and can be ahead of the runtime's own book-keeping of the events recorded in
// front of that kernel: hipEventElapsedTime then says "not ready" (once in two thousand calls, measured) — the events are
// waited for and asked again.
static hipError_t stage_elapsed(float* ms, hipEvent_t a, hipEvent_t b) {
  hipError_t e = hipEventElapsedTime(ms, a, b);
  if (e == hipErrorNotReady) {
    (void)hipGetLastError();
    e = hipEventSynchronize(a);
    if (e == hipSuccess) e = hipEventSynchronize(b);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, a, b);
  }
  return e;
}

// Stages [first, first + n) of a call whose events have all been recorded: their times join the handle's sums.
static int add_stage_times(plvs_tsdf_chisel* h, int first, int n) {
  for (int i = first; i < first + n; ++i) {
    float ms = 0.f;
    PLVS_HIP_TRY(stage_elapsed(&ms, h->ev[i], h->ev[i + 1]));
    h->stage_ms[i] += ms;
  }
  return PLVS_OK;
}
