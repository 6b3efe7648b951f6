// Kernels of the voxblox back end's ordered pipeline (host side: tsdf_voxblox_integrate.hpp): the poses of a call, the ray
// passes (count / fill) in their four flavours, the expansion of the sorted records into operands, the order-dependent fold
// (vb_chain_chunks), and the small kernels of the updated-block list and of upload_block.
#pragma once
#include "tsdf_voxblox_handle.hpp"

namespace {

constexpr int kMaxRaySteps = 1 << 16;

__device__ __forceinline__ PoseRt make_pose(const float* __restrict__ Twc, int c) {
  PoseRt p;
  const float* T = Twc + 12 * c;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) p.R[3 * i + j] = T[4 * i + j];
    p.t[i] = T[4 * i + 3];
  }
  quat_from_matrix(p.R, p.q);
  return p;
}

// The poses of a call with their quaternions, once per cloud (the kernels used to redo the conversion — a square root
// and a division — for every point and every voxel visit).
__global__ void vb_pose_prep(const float* __restrict__ Twc, int nclouds, PoseRt* __restrict__ poses) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nclouds) poses[c] = make_pose(Twc, c);
}

__device__ __forceinline__ PoseRt load_pose(const PoseRt* __restrict__ poses, int c) { return poses[c]; }

// Which point does sequence position i of the batch denote?
__device__ __forceinline__ int point_of_seq(const int32_t* __restrict__ offsets, int nclouds, int i,
                                            int* cloud) {
  const int c = cloud_of(offsets, nclouds, i);
  const int beg = offsets[c], cnt = offsets[c + 1] - beg;
  *cloud = c;
  return beg + (int)mixed_index((uint32_t)(i - beg), (uint32_t)cnt);
}

// The flavours of the ray passes.  kSimple: camera rays in the mixed visiting order.  kWorld: the
// world-cloud-with-normals flavour (make_ray_world): cloud order, no validity test; `aux` = normals, n x 3.  kMerged:
// MergedTsdfIntegrator's bundles in their integration order (make_ray_merged): xyz = merged points, `aux` = merged
// weights (n), `clr` = the bundles' clearing flags.
// kFast: FastTsdfIntegrator's rays (tsdf_voxblox_fast.hpp has decided which rays live and how many voxels each updates):
// the mixed order of kSimple, cast from the surface end, `aux` = the rays' update counts (uint32, 0 = no ray).
enum VbMode { kSimple = 0, kWorld = 1, kMerged = 2, kFast = 3 };

// The fill pass stages a wave's records in LDS: the 64 rays of a wave own ONE contiguous range of the record arrays
// (their counts were scanned in ray order), so the wave writes it with consecutive lanes on consecutive words instead of
// 64 lanes on 64 short pieces.  A wave whose range exceeds kFillStage records (carving) writes the excess directly.
constexpr int kFillStage = 1536;
template <bool kFill, int kMode>
__global__ __launch_bounds__(256) void vb_ray_pass(
    Params P, const float* __restrict__ xyz, const float* __restrict__ aux, const uint8_t* __restrict__ clr, int npoints,
    const int32_t* __restrict__ offsets, int nclouds, const PoseRt* __restrict__ Twc, Directory dir,
    VCounters* __restrict__ ctr, uint32_t* __restrict__ counts, uint32_t* __restrict__ rec_keys,
    uint32_t* __restrict__ rec_seq) {
  __shared__ uint32_t s_key[kFill ? 4 : 1][kFill ? kFillStage : 1], s_seq[kFill ? 4 : 1][kFill ? kFillStage : 1];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool valid = i < npoints;
  if (!kFill && !valid) return;
  uint32_t n = 0;
  const uint32_t out = (kFill && valid) ? counts[i] : 0u;
  // (lane 0 of a wave is valid whenever any lane is: the wave's range starts at its first ray's offset)
  const uint32_t wbase = kFill ? (uint32_t)__builtin_amdgcn_readfirstlane((int)out) : 0u;
  if (valid) {
    int cloud = 0;
    const int p = (kMode == kWorld || kMode == kMerged) ? i : point_of_seq(offsets, nclouds, i, &cloud);
    const float px = xyz[3 * (size_t)p], py = xyz[3 * (size_t)p + 1], pz = xyz[3 * (size_t)p + 2];
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) {
      // the reference filters such points out BEFORE the mixed order is formed;
      // PLVS's cloud generator never emits them, so refuse instead of diverging
      if (!kFill) atomicOr(&ctr->err, kErrNonFinite);
    } else {
      const PoseRt pose = load_pose(Twc, cloud);
      Ray ray;
      bool walk = true;
      if (kMode == kWorld) {
        float rs[3];
        make_ray_world(P, pose, px, py, pz, aux[3 * (size_t)p], aux[3 * (size_t)p + 1], aux[3 * (size_t)p + 2], &ray, rs);
      } else if (kMode == kMerged) {
        make_ray_merged(P, pose, px, py, pz, clr[p] != 0, &ray);
      } else {
        walk = make_ray(P, pose, px, py, pz, &ray, kMode == kFast);
      }
      uint32_t limit = 0xFFFFFFFFu;   // voxels the ray may update
      if (kMode == kFast) {
        limit = reinterpret_cast<const uint32_t*>(aux)[i];
        walk = walk && limit > 0u;
      }
      if (walk) {
        int lb[3] = {0, 0, 0}, lslot = -1;
        bool have_last = false;
        int steps = ray.steps < kMaxRaySteps ? ray.steps : kMaxRaySteps;
        if (kMode == kFast && (uint32_t)steps >= limit) steps = (int)limit - 1;
        for (int s = 0; s <= steps; ++s) {
          int g[3], b[3], vid;
          ray_step(&ray, g);
          const bool ok = block_of(P, g, b, &vid);   // no early continue: every lane takes one step per trip
          if (ok && (!have_last || b[0] != lb[0] || b[1] != lb[1] || b[2] != lb[2])) {
            lb[0] = b[0]; lb[1] = b[1]; lb[2] = b[2];
            have_last = true;
            if (kFill) {
              lslot = dir_find(dir, b[0], b[1], b[2]);
              if (lslot < 0) atomicOr(&ctr->err, kErrDirectoryMiss);
            } else {
              // the float block lookup left the integer grid, or the block lies where the binary32 voxel centre is no
              // longer the reference's (kBlockIdLimit): refused before it takes a slot
              if ((((g[0] - b[0] * 16) | (g[1] - b[1] * 16) | (g[2] - b[2] * 16)) & ~15) || !block_id_in_range(b[0], b[1], b[2]))
                atomicOr(&ctr->err, kErrCoordRange);
              else
                dir_insert(dir, b[0], b[1], b[2], &ctr->num_blocks, &ctr->err);
            }
          }
          if (ok && kFill) {
            // (a directory miss is an error the host reports: the record still gets a defined key)
            const uint32_t key = lslot >= 0 ? (uint32_t)lslot * (uint32_t)kBlockVox + (uint32_t)vid : 0u;
            const uint32_t at = out + n - wbase;
            if (at < (uint32_t)kFillStage) {
              s_key[wid][at] = key;
              s_seq[wid][at] = (uint32_t)i;
            } else {
              rec_keys[out + n] = key;
              rec_seq[out + n] = (uint32_t)i;
            }
          }
          n += ok ? 1u : 0u;
        }
      }
    }
  }
  if (!kFill) {
    counts[i] = n;
    return;
  }
  // the wave's staged records leave in one piece (a wave's LDS operations execute in order: no barrier)
  uint32_t wend = out + n;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) wend = max(wend, (uint32_t)__shfl_xor((int)wend, off));
  const uint32_t cnt = min(wend - wbase, (uint32_t)kFillStage);
  __builtin_amdgcn_wave_barrier();
  for (uint32_t j = (uint32_t)lane; j < cnt; j += 64u) {
    rec_keys[wbase + j] = s_key[wid][j];
    rec_seq[wbase + j] = s_seq[wid][j];
  }
}

constexpr int kExpandThreads = 1024;
template <int kMode>
__global__ __launch_bounds__(kExpandThreads) void vb_expand(
    Params P, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ seqs, uint32_t n,
    const float* __restrict__ xyz, const float* __restrict__ aux, const uint32_t* __restrict__ rgba,
    const int32_t* __restrict__ offsets, int nclouds, const PoseRt* __restrict__ Twc,
    const int32_t* __restrict__ slot_ids, float2* __restrict__ rec, uint32_t* __restrict__ rec_c,
    uint32_t* __restrict__ heads, uint32_t* __restrict__ updated_slots,
    VCounters* __restrict__ ctr) {
  __shared__ uint32_t wave_cnt[2][kExpandThreads / 64];
  __shared__ uint32_t block_base[2];
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  bool head = false, chead = false;
  uint32_t key = 0;
  if (r < n) {
    key = keys[r];
    const uint32_t prev = r ? keys[r - 1] : ~key;
    const uint32_t next = (r + 1 < n) ? keys[r + 1] : ~key;
    head = (r == 0) || (key != prev);
    chead = (r == 0) || ((key >> 12) != (prev >> 12));
    int cloud = 0;
    const int p = kMode != kSimple ? (int)seqs[r] : point_of_seq(offsets, nclouds, (int)seqs[r], &cloud);
    const PoseRt pose = load_pose(Twc, cloud);
    const float px = xyz[3 * (size_t)p], py = xyz[3 * (size_t)p + 1], pz = xyz[3 * (size_t)p + 2];
    const uint32_t slot = key >> 12, vid = key & 4095u;
    const int g[3] = {slot_ids[3 * slot + 0] * 16 + (int)(vid & 15u),
                      slot_ids[3 * slot + 1] * 16 + (int)((vid >> 4) & 15u),
                      slot_ids[3 * slot + 2] * 16 + (int)(vid >> 8)};
    float sdf, uw;
    if (kMode == kWorld) {   // updateTsdfVoxel(ray_start, point_G, ..., weight 1), tsdf_integrator.cc:78
      Ray ray;
      float rs[3];
      make_ray_world(P, pose, px, py, pz, aux[3 * (size_t)p], aux[3 * (size_t)p + 1], aux[3 * (size_t)p + 2], &ray, rs);
      visit_operands(P, rs, ray.pG, g, 1.0f, &sdf, &uw);
    } else if (kMode == kMerged) {   // updateTsdfVoxel(origin, merged_point_G, ..., merged_color, merged_weight), :443
      float pG[3];
      quat_transform(pose, px, py, pz, pG);
      visit_operands(P, pose.t, pG, g, aux[p], &sdf, &uw);
    } else {
      float pG[3];
      quat_transform(pose, px, py, pz, pG);
      const float weight = fabsf(pz) > 1e-6f ? 1.0f / (pz * pz) : 0.0f;
      visit_operands(P, pose.t, pG, g, weight, &sdf, &uw);
    }
    // The sign bit of the stored weight marks the LAST record of the voxel run, so the weight's own sign is cleared
    // first.  uw is never negative, but it can be -0.0: a point with |z| <= 1e-6 has weight 0, and behind the drop-off's
    // zero crossing 0 * (negative) / (positive) is -0.0, which std::max(uw, 0) keeps.  The sign of such a zero moves to
    // sdf: updateTsdfVoxel uses uw's sign only in the product sdf * uw (a weight sum or a blend factor takes +0.0 and
    // -0.0 alike, W being +0.0 or positive) and sdf, beside that product, only as fabsf(sdf); (-sdf) * +0.0 is
    // sdf * -0.0 bit for bit, so the folds give the reference's words — the sign of a zero distance included.
    if (__float_as_uint(uw) == 0x80000000u) sdf = -sdf;
    uw = fabsf(uw);
    rec[r] = make_float2(sdf, (key != next) ? -uw : uw);
    rec_c[r] = rgba[p];
  }
  const unsigned long long mh = __ballot(head), mc = __ballot(chead);
  if (lane == 0) {
    wave_cnt[0][wid] = (uint32_t)__popcll(mh);
    wave_cnt[1][wid] = (uint32_t)__popcll(mc);
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    uint32_t tot = 0;
    for (int w = 0; w < kExpandThreads / 64; ++w) {
      const uint32_t c = wave_cnt[threadIdx.x][w];
      wave_cnt[threadIdx.x][w] = tot;
      tot += c;
    }
    block_base[threadIdx.x] =
        tot ? atomicAdd(threadIdx.x == 0 ? &ctr->num_heads : &ctr->num_updated, tot) : 0u;
  }
  __syncthreads();
  if (head) heads[block_base[0] + wave_cnt[0][wid] + (uint32_t)__popcll(mh & lt)] = r;
  if (chead) updated_slots[block_base[1] + wave_cnt[1][wid] + (uint32_t)__popcll(mc & lt)] = key >> 12;
}

// The order-dependent fold of updateTsdfVoxel over the sorted records, record-centric: a workgroup takes kChainChunk
// consecutive records into LDS with coalesced loads and folds the voxel runs that START inside its chunk (a run that
// runs past the chunk's end reads on from global memory; one that started before belongs to the workgroup before).
// (The first version gave a thread one voxel run and read it at a stride of the run lengths: 12 B per visit in
// scattered pieces, 0.34 ms for the 11 M visits of a step.)
//
// Two ways to fold a run, by its length (round 3):
//  * SHORT runs (< kLongRun visits, wholly inside the chunk): a lane per run, voxel_fold visit by visit; a lane that
//    finishes takes the chunk's next short run at once.  In such a wave some lane starts a run in nearly every trip
//    of the loop, so a visit costs the wave the run-start path too (two global round trips): ≈ 0.6 us.  Fine for a few
//    visits — but a voxel that every key frame of the call sees has hundreds, and the kernel used to end with such
//    lanes (0.36 ms for 11 M visits).
//  * LONG runs (and the run that leaves the chunk): EIGHT lanes per run, eight visits per trip.  What makes a visit
//    expensive — three IEEE divisions, the byte <-> float conversions of four colour channels — does not depend on
//    the running distance or colour: the weight sequence W_k = min(W_{k-1} + w_k, max) only needs the records, and
//    with it the divisor (W_{k-1} + w_k), both blend factors and the product sdf*w of EVERY visit are known up front.
//    So per trip: the eight lanes take eight records; the weight chain runs through the eight visits (plain running
//    sums — the 1e-6 floor and the max_weight ceiling are checked afterwards and a trip they act on is redone);
//    lane g computes visit g's operands — one correctly rounded reciprocal and three exact quotients from it — into
//    LDS; then the order-dependent part runs with lane 0 carrying the distance (mul, add, the exact-quotient step
//    mul, fma, fma — dist_update_rcp's form — and a median for the clamp) and lanes 1-4 a colour channel each
//    (mul, add, round).  A trip of eight visits takes ≈ 1.3 us; nothing in it waits for global memory (the next
//    trip's records are fetched before the chains start, the voxels of all long runs are staged in LDS up front).
//    The groups take the chunk's long runs longest first, each the next one as soon as its own ends.
// Measured (MI355X, 25 key frames per call, 11.2 M visits): 0.36 -> 0.20 ms, the call 1.07 -> 0.92 ms.  The
// kernel is now bound by each chunk's longest run (a workgroup lives as long as it: ≈ 25 us on average, two to three
// times the 8 trips a group averages) at the four workgroups per CU its 40.8 KB of LDS allow (three at 45 KB: + 5 %).  Did not help: four
// lanes per run (slower: twice the trips on the critical run), 128- and 64-thread workgroups, a quarter fewer
// instructions per trip, a lane-path threshold anywhere from 8 to 128.
#ifndef PLVS_VB_LONG_RUN
#define PLVS_VB_LONG_RUN 16
#endif
constexpr int kChainChunk = 2048;
constexpr int kChainThreads = 256;
constexpr int kLongRun = PLVS_VB_LONG_RUN;
constexpr int kG = 8;   // lanes per long run = visits per trip
constexpr int kChainGroups = kChainThreads / kG;
constexpr int kMaxLong = kChainChunk / kLongRun + 2;

#ifndef PLVS_VB_PROF
#define PLVS_VB_PROF 0
#endif
#if PLVS_VB_PROF   // developer build: the times (100 MHz ticks) at which every wave passes its stages, read by plvs_hip_debug_chain_prof
constexpr int kProfWaves = 1 << 16;
__device__ unsigned long long g_chain_prof[kProfWaves][4];
#define CHAIN_PROBE(i)                                                                                         \
  if (lane == 0 && blockIdx.x * (kChainThreads / 64) + wid < kProfWaves)                                       \
    g_chain_prof[blockIdx.x * (kChainThreads / 64) + wid][i] = wall_clock64();
#else
#define CHAIN_PROBE(i)
#endif

// RN(1/b) for b in [2^-20, 2^40] (tsdf_chisel_ordered.hpp's rcp_rn: checked for every significand by plvs_hip_selftest_rcp) and
// RN(a/b) from it (dist_update_rcp's correction step), exact for a = 0 or |a| in [2^-60, 2^60]
__device__ __forceinline__ float vb_rcp_rn(float b) {
  const float y0 = __builtin_amdgcn_rcpf(b);
  const float e = fmaf(-b, y0, 1.0f);
  return fmaf(e, y0, y0);
}
__device__ __forceinline__ float vb_quot(float a, float b, float y) {
  const float q = a * y;
  const float r = fmaf(-q, b, a);
  return fmaf(r, y, q);
}
__device__ __forceinline__ bool vb_quot_ok(float a) { return a == 0.0f || (fabsf(a) >= 0x1p-60f && fabsf(a) <= 0x1p60f); }

// record rr of the chunk (LDS), of the records behind it (global) or a terminator beyond the call's last record
__device__ __forceinline__ void chain_load(const float2* s_rec, const uint32_t* s_col, const float2* __restrict__ rec,
                                           const uint32_t* __restrict__ rec_c, uint32_t c0, uint32_t n, uint32_t nrec,
                                           uint32_t rr, float2* v, uint32_t* col) {
  const uint32_t rl = min(rr, n - 1u);
  *v = s_rec[rl];
  *col = s_col[rl];
  if (rr >= n) {   // (only the run that leaves the chunk gets here)
    if (c0 + rr < nrec) {
      *v = rec[c0 + rr];
      *col = rec_c[c0 + rr];
    } else {
      *v = make_float2(0.f, -0.0f);
      *col = 0u;
    }
  }
}

__global__ __launch_bounds__(kChainThreads) void vb_chain_chunks(
    Params P, const uint32_t* __restrict__ keys, uint32_t nrec, const float2* __restrict__ rec,
    const uint32_t* __restrict__ rec_c, VCounters* __restrict__ ctr, float* __restrict__ dist,
    float* __restrict__ weight, uint32_t* __restrict__ rgba) {
  __shared__ float2 s_rec[kChainChunk];
  __shared__ uint32_t s_col[kChainChunk];
  __shared__ uint16_t s_head[kChainChunk + 2];   // positions of the run heads of the chunk, ascending; then the chunk's end
  __shared__ uint16_t s_long[kMaxLong];          // the long ones
  __shared__ unsigned long long s_mask[kChainChunk / 64];
  __shared__ uint32_t s_pre[kChainChunk / 64];
  // the per-visit operands of a trip, the distance lane's and the colour lanes' apart
  // (40.8 KB in all: four workgroups per CU.  The short runs' list lies over the distance operands — it is dead before the
  // long loop's first trip, a barrier between — and the operand rows are unpadded: the bank conflicts of the groups'
  // broadcast reads cost 1 %, the fourth workgroup gains 5 % of the call.  Chunks of 1536 / 1024 records: slower.)
  __shared__ float4 s_opd[kChainGroups][kG], s_opc[kChainGroups][kG];
  static_assert(sizeof(s_opd) >= kChainChunk * sizeof(uint16_t), "the short runs' list lies over the distance operands");
  uint16_t* const s_short = reinterpret_cast<uint16_t*>(&s_opd[0][0]);   // the short runs (indices into s_head), any order
  __shared__ __attribute__((aligned(16))) float s_uw[kChainGroups][kG];
  __shared__ float4 s_state[kMaxLong];           // a long run's voxel: distance, weight, colour, its index in the pool
  __shared__ uint32_t s_cls[32];
  __shared__ uint32_t s_nheads, s_nshort, s_nlong, s_next, s_next_long;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const uint32_t c0 = blockIdx.x * (uint32_t)kChainChunk;
  if (c0 >= nrec) return;
  const uint32_t n = min((uint32_t)kChainChunk, nrec - c0);
  CHAIN_PROBE(0)
  if (tid < 32) s_cls[tid] = 0;
  if (tid == 0) {
    s_nshort = 0;
    s_nlong = 0;
    s_next = (uint32_t)kChainThreads;   // the next short run to hand out; the first ones go by thread index
    s_next_long = (uint32_t)kChainGroups;   // the same for long runs and groups
  }
  // ---- the chunk into LDS; its run heads in record order.  All loads of the thread are issued before the first is
  // used (clamped addresses instead of branches): one memory latency per chunk, not one per round.
  constexpr int kRounds = kChainChunk / kChainThreads;
  float2 l_rec[kRounds];
  uint32_t l_col[kRounds], l_key[kRounds], l_prev[kRounds];
#pragma unroll
  for (int k = 0; k < kRounds; ++k) {
    const uint32_t at = c0 + min((uint32_t)(k * kChainThreads + tid), n - 1u);
    l_rec[k] = rec[at];
    l_col[k] = rec_c[at];
    l_key[k] = keys[at];
    l_prev[k] = keys[max(at, 1u) - 1u];
  }
  uint32_t myheads = 0;
#pragma unroll
  for (int k = 0; k < kRounds; ++k) {
    const uint32_t r = (uint32_t)(k * kChainThreads + tid);
    bool head = false;
    if (r < n) {
      s_rec[r] = l_rec[k];
      s_col[r] = l_col[k];
      head = (c0 + r == 0u) || l_prev[k] != l_key[k];
    }
    const unsigned long long m = __ballot(head);
    if (lane == 0) s_mask[k * (kChainThreads / 64) + wid] = m;
    myheads |= head ? (1u << k) : 0u;
  }
  __syncthreads();
  if (tid < kChainChunk / 64) {   // (32 words: half of wave 0)
    const uint32_t c = (uint32_t)__popcll(s_mask[tid]);
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < kChainChunk / 64; off <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
      if (tid >= off) incl += up;
    }
    s_pre[tid] = incl - c;
    if (tid == kChainChunk / 64 - 1) s_nheads = incl;
  }
  __syncthreads();
  const uint32_t nheads = s_nheads;
#pragma unroll
  for (int k = 0; k < kChainChunk / kChainThreads; ++k) {
    if ((myheads >> k) & 1u) {
      const int w = k * (kChainThreads / 64) + wid;
      s_head[s_pre[w] + (uint32_t)__popcll(s_mask[w] & lt)] = (uint16_t)(k * kChainThreads + tid);
    }
  }
  if (tid == 0) s_head[nheads] = (uint16_t)n;
  __syncthreads();
  // ---- short and long runs.  The chunk's last run is long when it goes on behind the chunk.  The long ones are put
  // in classes of descending length (a counting sort over trips of eight visits; the run that leaves the chunk first):
  // the groups take them in that order, so a workgroup does not end with one group on a long run it started last.
  const bool crossing = !(__float_as_uint(s_rec[n - 1u].y) >> 31);
  auto run_class = [&](uint32_t h, bool* is_long) -> uint32_t {
    const uint32_t len = (uint32_t)s_head[h + 1u] - (uint32_t)s_head[h];
    const bool leaves = crossing && h + 1u == nheads;
    *is_long = len >= (uint32_t)kLongRun || leaves;
    return leaves ? 0u : 31u - min((len + 7u) >> 3, 31u);
  };
  for (uint32_t base = 0; base < nheads; base += (uint32_t)kChainThreads) {
    const uint32_t h = base + (uint32_t)tid;
    bool is_long = false, is_short = false;
    if (h < nheads) {
      const uint32_t cls = run_class(h, &is_long);
      is_short = !is_long;
      if (is_long) atomicAdd(&s_cls[cls], 1u);
    }
    const unsigned long long ms = __ballot(is_short);
    uint32_t bs = 0;
    if (lane == 0 && ms) bs = atomicAdd(&s_nshort, (uint32_t)__popcll(ms));
    bs = (uint32_t)__shfl((int)bs, 0);
    if (is_short) s_short[bs + (uint32_t)__popcll(ms & lt)] = (uint16_t)h;
  }
  __syncthreads();
  if (tid < 32) {
    const uint32_t c = s_cls[tid];
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
      if (tid >= off) incl += up;
    }
    s_cls[tid] = incl - c;   // (from here on: where the class's next run goes)
    if (tid == 31) s_nlong = incl;
  }
  __syncthreads();
  for (uint32_t base = 0; base < nheads; base += (uint32_t)kChainThreads) {
    const uint32_t h = base + (uint32_t)tid;
    if (h < nheads) {
      bool is_long;
      const uint32_t cls = run_class(h, &is_long);
      if (is_long) s_long[atomicAdd(&s_cls[cls], 1u)] = (uint16_t)h;
    }
  }
  __syncthreads();
  const uint32_t nshort = s_nshort, nlong = s_nlong;
  uint32_t longest = 0;
  // the voxels of the long runs into LDS, all loads side by side (a group that starts a run inside the trip loop below
  // must not make its wave wait for global memory)
  for (uint32_t j = (uint32_t)tid; j < nlong; j += (uint32_t)kChainThreads) {
    const uint32_t a = keys[c0 + s_head[s_long[j]]];
    s_state[j] = make_float4(dist[a], weight[a], __uint_as_float(rgba[a]), __uint_as_float(a));
  }
  CHAIN_PROBE(1)
  // ---- short runs: a lane per run
  {
    uint32_t i = (uint32_t)tid, r = 0;
    size_t a = 0;
    float D = 0.f, W = 0.f;
    uint32_t C = 0;
    bool have = false;
    for (;;) {
      if (!have) {
        if (i >= nshort) break;
        const uint32_t h = s_short[i];
        r = s_head[h];
        longest = max(longest, (uint32_t)s_head[h + 1u] - r);
        a = (size_t)keys[c0 + r];
        D = dist[a];
        W = weight[a];
        C = rgba[a];
        have = true;
      }
      const float2 v = s_rec[r];
      voxel_fold(P, D, W, C, v.x, fabsf(v.y), s_col[r]);
      if (__float_as_uint(v.y) >> 31) {   // (its sign bit marks the last record of the run)
        dist[a] = D;
        weight[a] = W;
        rgba[a] = C;
        have = false;
        i = atomicAdd(&s_next, 1u);
      } else {
        ++r;
      }
    }
  }
  CHAIN_PROBE(2)
  // ---- long runs: kG lanes per run, kG visits per trip.  Lane 0 of the group carries the distance, lanes 1-4 a colour
  // channel each.  ONE loop: a group whose run ends takes the
  // chunk's next long run in the same trip, so the groups of a wave never wait for each other's runs.
  __syncthreads();   // (s_state complete)
  const int grp = tid / kG, g = tid % kG;
  const int sh = 8 * ((g - 1) & 3);   // lanes 1-4 (and, idle, 0 and 5-7): the colour channel
  {
    // (the first runs — the longest — dealt round the waves, not eight in a row to each: a workgroup's waves sit on
    // different SIMDs)
    constexpr int kGroupsPerWave = 64 / kG, kWaves = kChainThreads / 64;
    uint32_t j = (uint32_t)((grp % kGroupsPerWave) * kWaves + grp / kGroupsPerWave), r = 0, visits = 0, col = 0;
    float W = 0.f, X = 0.f, Dx = 0.f;
    float2 v = make_float2(0.f, 0.f);
    bool have = false;
    for (;;) {
      if (!have) {
        if (j >= nlong) break;
        const float4 st = s_state[j];
        Dx = st.x;                                              // (lane 0's)
        W = st.y;
        X = (float)((__float_as_uint(st.z) >> sh) & 255u);      // the lane's colour channel
        r = s_head[s_long[j]];
        visits = 0;
        chain_load(s_rec, s_col, rec, rec_c, c0, n, nrec, r + (uint32_t)g, &v, &col);
        have = true;
      }
      // the visits of this trip: up to the run's last record
      const unsigned long long bal = __ballot(__float_as_uint(v.y) >> 31);
      const uint32_t gm = (uint32_t)(bal >> (lane & ~(kG - 1))) & ((1u << kG) - 1u);
      const int nvalid = gm ? __ffs((int)gm) : kG;
      const bool done = gm != 0u;
      const float sdf = v.x, uw = fabsf(v.y);
      s_uw[grp][g] = uw;
      float2 vn = make_float2(0.f, 0.f);
      uint32_t coln = 0;
      if (!done) chain_load(s_rec, s_col, rec, rec_c, c0, n, nrec, r + (uint32_t)(kG + g), &vn, &coln);
      __builtin_amdgcn_wave_barrier();
      // the weight chain: lane g takes the steps of the visits before its own
      float u[kG];
#pragma unroll
      for (int k = 0; k < kG; k += 4)
        *reinterpret_cast<float4*>(&u[k]) = *reinterpret_cast<const float4*>(&s_uw[grp][k]);
      // (plain running sums first: the 1e-6 floor and the max_weight ceiling of updateTsdfVoxel almost never act, and a
      // lane whose own sum is clean knows that the sums before it were)
      float w_prev = W;
#pragma unroll
      for (int k = 0; k < kG - 1; ++k) {
        const float nwk = w_prev + u[k];
        w_prev = (k < g) ? nwk : w_prev;
      }
      float nw = w_prev + uw;
      {
        const unsigned long long balw = __ballot((g < nvalid) && !((nw >= 1e-6f) && (nw < P.max_weight)));
        if ((((uint32_t)(balw >> (lane & ~(kG - 1)))) & ((1u << kG) - 1u)) != 0u) {
          w_prev = W;
          for (int k = 0; k < kG - 1; ++k) {
            const float nwk = w_prev + u[k];
            const float stepped = (nwk < 1e-6f) ? w_prev : ((nwk < P.max_weight) ? nwk : P.max_weight);
            w_prev = (k < g) ? stepped : w_prev;
          }
          nw = w_prev + uw;
        }
      }
      const bool skip = (g >= nvalid) || (nw < 1e-6f);
      const float w_after = skip ? w_prev : ((nw < P.max_weight) ? nw : P.max_weight);
      W = __shfl(w_after, nvalid - 1, kG);   // (the weight after the trip's last visit)
      // visit g's operands (blend_colours' total = w1 + w2 is nw): the distance half, the colour half
      const bool rcp_ok = (nw >= 0x1p-20f) && (nw <= 0x1p40f);
      const unsigned long long balr = __ballot(!skip && !rcp_ok);
      bool inexact = (((uint32_t)(balr >> (lane & ~(kG - 1)))) & ((1u << kG) - 1u)) != 0u;
      {
        const bool blend = !skip && (fabsf(sdf) < P.truncation);
        // 1 / nw correctly rounded (v_rcp_f32 and one Newton step: plvs_hip_selftest_rcp), and both blend factors as exact
        // quotients from it (the same correction step as the distance's); operands outside the exact ranges divide
        float y = vb_rcp_rn(nw), w1n = vb_quot(w_prev, nw, y), w2n = vb_quot(uw, nw, y);
        if (!skip && !(rcp_ok && vb_quot_ok(w_prev) && vb_quot_ok(uw))) {   // (a skipped visit's operands are not used)
          y = 1.0f / nw;
          w1n = w_prev / nw;
          w2n = uw / nw;
        }
        s_opd[grp][g] = make_float4(skip ? -fabsf(w_prev) : fabsf(w_prev), sdf * uw, y, nw);   // (an uploaded weight can be -0.0)
        s_opc[grp][g] = make_float4(w1n, w2n, __uint_as_float(col), blend ? 1.0f : 0.0f);
      }
      __builtin_amdgcn_wave_barrier();
      float4 opc[kG];
#pragma unroll
      for (int k = 0; k < kG; ++k) opc[k] = s_opc[grp][k];
      // the order-dependent part.  A colour step: round(a*w1 + b*w2) of non-negative operands with w1 + w2 = 1 up to
      // roundings is an integer in [0, 255] — blend_colours' cast to a byte and back changes nothing.
      auto colour_steps = [&](float x) {
#pragma unroll
        for (int k = 0; k < kG; ++k) {
          const float b = (float)((__float_as_uint(opc[k].z) >> sh) & 255u);
          const float t = x * opc[k].x + b * opc[k].y;
          const float tr = truncf(t);
          const float nc = tr + (((t - tr) >= 0.5f) ? 1.0f : 0.0f);   // roundf of t >= 0
          x = (opc[k].w != 0.0f) ? nc : x;
        }
        return x;
      };
      if (g == 0) {
        float4 opd[kG];
#pragma unroll
        for (int k = 0; k < kG; ++k) opd[k] = s_opd[grp][k];
        // (the quotient from the reciprocal is exact inside dist_update_rcp_exact's operand ranges; a trip that leaves
        // them — none does on real data — is redone with the division itself)
        const float x0 = Dx;
#pragma unroll
        for (int k = 0; k < kG; ++k) {
          const bool skipk = __float_as_uint(opd[k].x) >> 31;
          const float t = opd[k].y + Dx * fabsf(opd[k].x);   // sdf * w + D * W
          const float y = opd[k].z, nwk = opd[k].w;
          const float q = t * y;
          const float rem = fmaf(-q, nwk, t);
          const float nd = fmaf(rem, y, q);
          const float at = fabsf(t);
          inexact |= !skipk && !(at >= 0x1p-60f && at <= 0x1p60f);
          // (an exact quotient of in-range operands is finite: the median IS voxel_fold's pair of std::min / std::max)
          Dx = skipk ? Dx : __builtin_amdgcn_fmed3f(nd, -P.truncation, P.truncation);
        }
        if (inexact) {
          Dx = x0;
          for (int k = 0; k < kG; ++k) {
            const float t = opd[k].y + Dx * fabsf(opd[k].x);
            float nd = t / opd[k].w;
            nd = (nd > 0.0f) ? ((nd < P.truncation) ? nd : P.truncation) : ((-P.truncation < nd) ? nd : -P.truncation);
            Dx = (__float_as_uint(opd[k].x) >> 31) ? Dx : nd;
          }
        }
      } else {
        X = colour_steps(X);
      }
      __builtin_amdgcn_wave_barrier();
      visits += (uint32_t)nvalid;
      if (done) {
        const uint32_t cx = (uint32_t)X;
        const uint32_t C = (uint32_t)__shfl((int)cx, 1, kG) | ((uint32_t)__shfl((int)cx, 2, kG) << 8) |
                           ((uint32_t)__shfl((int)cx, 3, kG) << 16) | ((uint32_t)__shfl((int)cx, 4, kG) << 24);
        uint32_t jn = 0;
        if (g == 0) {
          s_state[j] = make_float4(Dx, W, __uint_as_float(C), s_state[j].w);
          jn = atomicAdd(&s_next_long, 1u);
        }
        j = (uint32_t)__shfl((int)jn, 0, kG);
        longest = max(longest, visits);
        have = false;
      } else {
        v = vn;
        col = coln;
        r += (uint32_t)kG;
      }
    }
  }
  __syncthreads();
  for (uint32_t j = (uint32_t)tid; j < nlong; j += (uint32_t)kChainThreads) {
    const float4 st = s_state[j];
    const size_t a = (size_t)__float_as_uint(st.w);
    dist[a] = st.x;
    weight[a] = st.y;
    rgba[a] = __float_as_uint(st.z);
  }
  CHAIN_PROBE(3)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, off));
  if (lane == 0 && longest > ctr->max_run) atomicMax(&ctr->max_run, longest);
}

// The updated-block list without the blocks that have not joined the layer yet (slots >= visible), order kept; one
// workgroup (the list has a few thousand entries).  *n_out = the new length.
__global__ __launch_bounds__(1024) void vb_filter_slots(uint32_t* __restrict__ slots, uint32_t n, uint32_t visible,
                                                        uint32_t* __restrict__ n_out) {
  __shared__ uint32_t s_cnt[16];
  __shared__ uint32_t s_base;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) s_base = 0u;
  __syncthreads();
  for (uint32_t i0 = 0; i0 < n; i0 += 1024u) {
    const uint32_t i = i0 + (uint32_t)tid;
    const uint32_t v = i < n ? slots[i] : 0u;
    const bool keep = i < n && v < visible;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_cnt[wid] = (uint32_t)__popcll(m);
    __syncthreads();   // (every slot of this round has been read: compaction only moves entries towards the front)
    uint32_t at = s_base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wid; ++w) at += s_cnt[w];
    if (keep) slots[at] = v;
    __syncthreads();
    if (tid == 0) {
      uint32_t t = 0;
      for (int w = 0; w < 16; ++w) t += s_cnt[w];
      s_base += t;
    }
    __syncthreads();
  }
  if (tid == 0) *n_out = s_base;
}

__global__ void vb_gather_slot_ids(const uint32_t* __restrict__ slots, int n,
                                   const int32_t* __restrict__ slot_ids, int32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const uint32_t s = slots[i];
    out[3 * i] = slot_ids[3 * s];
    out[3 * i + 1] = slot_ids[3 * s + 1];
    out[3 * i + 2] = slot_ids[3 * s + 2];
  }
}

// One block id -> its pool slot, created if absent (plvs_hip_tsdf_voxblox_upload_block).
__global__ void vb_block_slot_of(Directory dir, int x, int y, int z, VCounters* __restrict__ ctr, int32_t* __restrict__ slot_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (!block_id_in_range(x, y, z)) {   // (a block no integrate would accept)
    atomicOr(&ctr->err, kErrCoordRange);
    *slot_out = -1;
    return;
  }
  dir_insert(dir, x, y, z, &ctr->num_blocks, &ctr->err);
  *slot_out = dir_find(dir, x, y, z);
}

}  // namespace
