// TSDF map of the open_chisel back end (PointCloudMapChisel): the C ABI of the map handle.  This file keeps the handle's
// life cycle, the integrate entry points and their queue, the accessors and the self-tests; each pipeline that works on
// the handle has a header of its own, all compiled into this one translation unit (the walk's templated kernels are
// instantiated from headers: a second unit would instantiate them again):
//   tsdf_chisel_handle.hpp      the handle, its counters and their reads, stage times, failure paths
//   tsdf_chisel_ordered.hpp     ordered mode: bit-identical to the reference's sequential loop (ray_count ... chain_runs)
//   tsdf_chisel_order_free.hpp  order-free mode: the single-walk pipeline of tsdf_walk.hpp, planned by tsdf_walk_plan.hpp
//   tsdf_chisel_shard.hpp       ray-sharded multi-GPU integrate (kernels: tsdf_shard.hpp)
//   tsdf_chisel_carve.hpp       carving
//   tsdf_chisel_halo.hpp        halo of a sharded map (meshing)
//   tsdf_chisel_deform.hpp      Chisel::Deform
//   tsdf_chisel_scan.hpp        projective depth + colour scan integrate
#include "tsdf_chisel_handle.hpp"
#include "tsdf_chisel_halo.hpp"
#include "tsdf_chisel_ordered.hpp"
#include "tsdf_chisel_order_free.hpp"
#include "tsdf_chisel_carve.hpp"
#include "tsdf_chisel_shard.hpp"
#include "tsdf_chisel_deform.hpp"
#include "tsdf_chisel_scan.hpp"

namespace {

__global__ void pool_init(float* __restrict__ sdf, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t j = i; j < n; j += stride) sdf[j] = 99999.0f;
}

// Self-test of the device-wide stable radix sort (device_utils.hip) at sizes on both sides of its two scatter paths:
// pseudo-random keys below 2^bits (many equal keys when bits is small), values = original positions.
__global__ void selftest_sort_fill(uint32_t* __restrict__ keys, uint32_t* __restrict__ v32, unsigned long long* __restrict__ v64,
                                   uint32_t n, int bits, uint32_t seed) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t x = (i + 1u) * 2654435761u + seed;
  x ^= x << 13; x ^= x >> 17; x ^= x << 5;
  x ^= x << 13; x ^= x >> 17; x ^= x << 5;
  keys[i] = bits >= 32 ? x : (x & ((1u << bits) - 1u));
  if (v32) v32[i] = i;
  if (v64) v64[i] = ((unsigned long long)~i << 32) | i;
}
// mismatches[0]: order / stability violations, [1]: a pair whose key is not the key its value's position held
__global__ void selftest_sort_check(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ keys,
                                    const uint32_t* __restrict__ v32, const unsigned long long* __restrict__ v64, uint32_t n,
                                    int bit_lo, int bit_hi, uint32_t* __restrict__ mismatches) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t mask = (bit_hi - bit_lo >= 32 ? 0xFFFFFFFFu : ((1u << (bit_hi - bit_lo)) - 1u)) << bit_lo;
  const uint32_t pos = v32 ? v32[i] : (uint32_t)v64[i];
  if (pos >= n || keys_in[pos] != keys[i] || (v64 && (uint32_t)(v64[i] >> 32) != ~pos)) atomicAdd(&mismatches[1], 1u);
  if (i + 1 < n) {
    const uint32_t a = keys[i] & mask, b = keys[i + 1] & mask;
    const uint32_t pn = v32 ? v32[i + 1] : (uint32_t)v64[i + 1];
    if (a > b || (a == b && pos >= pn)) atomicAdd(&mismatches[0], 1u);
  }
}

// Hardware assumption of chain_runs, checked exhaustively: rcp_rn(b) == RN(1/b) for every
// significand at the given exponent.
__global__ void selftest_rcp_kernel(int exponent, uint32_t* __restrict__ mismatches) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  const float b = __uint_as_float(((uint32_t)(exponent + 127) << 23) | m);
  if (__float_as_uint(rcp_rn(b)) != __float_as_uint(1.0f / b)) atomicAdd(mismatches, 1u);
}

}  // namespace

// The reference's cloud of every depth image of a call, for the handles that take point streams (ordered / sharded /
// deform-tracking): cell = (image, grid pixel) in raster order; mark -> exclusive scan -> emit.
__global__ __launch_bounds__(256) void grid_cloud_mark(GridSrc g, int nclouds, uint32_t* __restrict__ flag) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, ngrid = (size_t)g.gw * g.gh;
  if (i >= ngrid * (size_t)nclouds) return;
  const uint32_t c = (uint32_t)(i / ngrid), r = (uint32_t)(i - (size_t)c * ngrid), m = r / g.gw, n = r - m * g.gw;
  const float d = g.depth[(size_t)c * g.image_stride + (size_t)(m * g.step) * g.pitch + n * g.step];
  flag[i] = (((double)d > g.min_depth) && ((double)d < g.max_depth)) ? 1u : 0u;   // src/PointCloudMapping.cc:967
}
__global__ __launch_bounds__(256) void grid_cloud_emit(GridSrc g, int nclouds, const uint32_t* __restrict__ pos /* cells + 1 */,
                                                       const uint8_t* __restrict__ bgr, const uint32_t* __restrict__ kfid_of_image,
                                                       float* __restrict__ xyz, uint8_t* __restrict__ rgb,
                                                       uint32_t* __restrict__ kfid, uint32_t* __restrict__ offsets) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, ngrid = (size_t)g.gw * g.gh, cells = ngrid * (size_t)nclouds;
  if (i > cells) return;
  if (i == cells || i % ngrid == 0) offsets[i / ngrid] = pos[i];
  if (i == cells || pos[i + 1] == pos[i]) return;
  const uint32_t c = (uint32_t)(i / ngrid), r = (uint32_t)(i - (size_t)c * ngrid), m = r / g.gw, n = r - m * g.gw;
  const float d = g.depth[(size_t)c * g.image_stride + (size_t)(m * g.step) * g.pitch + n * g.step];
  const float2 cam = reinterpret_cast<const float2*>(g.cam)[r];
  const size_t o = pos[i];
  xyz[3 * o] = cam.x * d;        // :973-975
  xyz[3 * o + 1] = cam.y * d;
  xyz[3 * o + 2] = d;
  const uint8_t* px = bgr + (size_t)c * g.bgr_image_stride + (size_t)(m * g.step) * g.bgr_pitch + (size_t)(n * g.step) * 3u;
  rgb[3 * o] = px[0];            // :978-980: the point's r, g, b members take bytes 0, 1, 2 of the pixel
  rgb[3 * o + 1] = px[1];
  rgb[3 * o + 2] = px[2];
  kfid[o] = kfid_of_image ? kfid_of_image[c] : 0u;
}

extern "C" {

int plvs_hip_selftest_rcp(int exponent, uint32_t* mismatches) {
  PLVS_REQUIRE(mismatches && exponent > -126 && exponent < 127, "bad argument");
  uint32_t* d = nullptr;
  PLVS_HIP_TRY(hipMalloc((void**)&d, sizeof(uint32_t)));
  PLVS_HIP_TRY(hipMemset(d, 0, sizeof(uint32_t)));
  hipLaunchKernelGGL(selftest_rcp_kernel, dim3((1u << 23) / 256), dim3(256), 0, nullptr, exponent, d);
  hipError_t e = hipMemcpy(mismatches, d, sizeof(uint32_t), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  PLVS_HIP_TRY(e);
  return PLVS_OK;
}

int plvs_hip_selftest_radix_sort(uint32_t n, int bit_lo, int bit_hi, int wide_values, uint32_t seed, uint32_t* mismatches2) {
  PLVS_REQUIRE(mismatches2 && n > 0 && bit_lo >= 0 && bit_hi > bit_lo && bit_hi <= 32, "bad argument");
  plvs::DevBuf<uint32_t> k_in, k0, k1, v0, v1, scratch, bad;
  plvs::DevBuf<unsigned long long> w0, w1;
  // wide_values = 2: the sort launched on a BOUND of the number of pairs (radix_sort_pairs_bound): the arrays are sized for
  // n + n / 2 + 4097 pairs, the first n are filled, the count sits in a device word
  const bool bound_mode = wide_values == 2;
  if (bound_mode) wide_values = 0;
  const uint32_t n_alloc = bound_mode ? n + n / 2 + 4097u : n;
  PLVS_HIP_TRY(k_in.reserve(n_alloc));
  PLVS_HIP_TRY(k0.reserve(n_alloc));
  PLVS_HIP_TRY(k1.reserve(n_alloc));
  if (wide_values) {
    PLVS_HIP_TRY(w0.reserve(n));
    PLVS_HIP_TRY(w1.reserve(n));
  } else {
    PLVS_HIP_TRY(v0.reserve(n_alloc));
    PLVS_HIP_TRY(v1.reserve(n_alloc));
  }
  PLVS_HIP_TRY(scratch.reserve(radix_scratch_words(n_alloc) + 1));
  PLVS_HIP_TRY(bad.reserve(2));
  PLVS_HIP_TRY(hipMemset(bad.p, 0, 2 * sizeof(uint32_t)));
  const dim3 grid(ceil_div((size_t)n, 256)), block(256);
  hipLaunchKernelGGL(selftest_sort_fill, grid, block, 0, nullptr, k0.p, v0.p, w0.p, n, bit_hi, seed);
  PLVS_HIP_TRY(hipMemcpyAsync(k_in.p, k0.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, nullptr));
  bool second = false;
  if (bound_mode) {
    PLVS_HIP_TRY(hipMemsetAsync(k0.p + n, 0x5A, (size_t)(n_alloc - n) * sizeof(uint32_t), nullptr));   // (what lies behind the pairs is not sorted in)
    uint32_t* d_n = scratch.p + radix_scratch_words(n_alloc);
    PLVS_HIP_TRY(hipMemcpyAsync(d_n, &n, sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
    PLVS_HIP_TRY(hipStreamSynchronize(nullptr));
    PLVS_HIP_TRY(radix_sort_pairs_bound(k0.p, v0.p, k1.p, v1.p, n_alloc, d_n, bit_lo, bit_hi, scratch.p, nullptr, &second));
  } else if (wide_values) PLVS_HIP_TRY(radix_sort_pairs_u64(k0.p, w0.p, k1.p, w1.p, n, bit_lo, bit_hi, scratch.p, nullptr, &second));
  else PLVS_HIP_TRY(radix_sort_pairs(k0.p, v0.p, k1.p, v1.p, n, bit_lo, bit_hi, scratch.p, nullptr, &second));
  hipLaunchKernelGGL(selftest_sort_check, grid, block, 0, nullptr, k_in.p, second ? k1.p : k0.p,
                     wide_values ? (const uint32_t*)nullptr : (second ? v1.p : v0.p),
                     wide_values ? (second ? w1.p : w0.p) : (const unsigned long long*)nullptr, n, bit_lo, bit_hi, bad.p);
  hipError_t e = hipMemcpy(mismatches2, bad.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost);
  k_in.release(); k0.release(); k1.release(); v0.release(); v1.release(); w0.release(); w1.release(); scratch.release(); bad.release();
  PLVS_HIP_TRY(e);
  return PLVS_OK;
}

#ifdef PLVS_WALK_PROF
// developer build only (make PROF=1): the phase clocks of walk_tiles, summed over the tiles since the last reset
int plvs_hip_debug_walk_prof(unsigned long long* out16, int reset) {
  if (out16) PLVS_HIP_TRY(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_walk_prof), 16 * sizeof(unsigned long long)));
  if (reset) {
    unsigned long long z[16] = {};
    PLVS_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_walk_prof), z, sizeof z));
  }
  return PLVS_OK;
}
#endif

int plvs_hip_selftest_walk_math(uint32_t seed, uint32_t* mismatches_sqrt_div) {
  PLVS_REQUIRE(mismatches_sqrt_div, "null argument");
  uint32_t* d = nullptr;
  PLVS_HIP_TRY(hipMalloc((void**)&d, 2 * sizeof(uint32_t)));
  PLVS_HIP_TRY(hipMemset(d, 0, 2 * sizeof(uint32_t)));
  hipLaunchKernelGGL(selftest_walk_math_kernel, dim3(16384), dim3(256), 0, nullptr, seed, d);
  hipError_t e = hipMemcpy(mismatches_sqrt_div, d, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  PLVS_HIP_TRY(e);
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_default_params(float resolution, plvs_tsdf_chisel_params* p) {
  PLVS_REQUIRE(p, "params is null");
  PLVS_REQUIRE(resolution > 0.0f, "resolution must be positive");
  p->resolution = resolution;
  p->trunc_quad = 0.0019f;      // ChiselServer.cpp:56-59
  p->trunc_linear = -0.00152f;
  p->trunc_const = 0.001504f;
  p->trunc_scale = 6.0f;
  p->weight = 1.0f;             // ChiselServer.cpp:60 (uint16_t weight = 1)
  p->max_chunks = 32768;        // 2 GiB of voxel pool
  p->shard_rank = 0;
  p->shard_count = 1;
  p->order_free = 0;
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_create(const plvs_tsdf_chisel_params* p, plvs_tsdf_chisel** out) {
  PLVS_REQUIRE(p && out, "null argument");
  PLVS_REQUIRE(p->resolution > 0.0f, "resolution must be positive");
  PLVS_REQUIRE(p->max_chunks > 0 && p->max_chunks <= (1 << 20), "max_chunks must be in (0, 2^20]");
  PLVS_REQUIRE(p->shard_count <= 1 || (p->shard_rank >= 0 && p->shard_rank < p->shard_count),
               "shard_rank out of range");
  plvs_tsdf_chisel* h = new plvs_tsdf_chisel();
  h->prm = *p;
  Params& P = h->P;
  P.resolution = p->resolution;
  P.round_to_voxel = 1.0f / p->resolution;                                   // Chisel.cpp:444
  P.half_voxel = p->resolution * 0.5f;                                       // ChunkManager.cpp:68
  P.rounding = 1.0f / ((float)16 * p->resolution);                           // ChunkManager.cpp:91
  P.diag = (float)(2.0 * std::sqrt((double)3.0f) * (double)p->resolution);   // Chisel.cpp:447
  P.tq = p->trunc_quad; P.tl = p->trunc_linear; P.tc = p->trunc_const; P.ts = p->trunc_scale;
  P.weight = p->weight;
  P.shard_rank = p->shard_rank;
  P.shard_count = p->shard_count < 1 ? 1 : p->shard_count;

  uint32_t cap = 1024;
  while (cap < 2u * (uint32_t)p->max_chunks) cap <<= 1;
  h->dir.mask = cap - 1;
  h->dir.max_blocks = p->max_chunks;
  const size_t nvox = (size_t)p->max_chunks * kChunkVox;
#define CREATE_TRY(call)                                                        \
  do {                                                                          \
    hipError_t _e = (call);                                                     \
    if (_e != hipSuccess) {                                                     \
      plvs::set_error("%s failed: %s", #call, hipGetErrorString(_e));          \
      plvs_hip_tsdf_chisel_destroy(h);                                          \
      return PLVS_ERR_HIP;                                                      \
    }                                                                           \
  } while (0)
  CREATE_TRY(hipMalloc((void**)&h->dir.keys, (size_t)cap * sizeof(unsigned long long)));
  CREATE_TRY(hipMalloc((void**)&h->dir.slots, (size_t)cap * sizeof(int32_t)));
  CREATE_TRY(hipMalloc((void**)&h->dir.slot_ids, (size_t)p->max_chunks * 3 * sizeof(int32_t)));
  CREATE_TRY(hipMalloc((void**)&h->sdf, nvox * sizeof(float)));
  CREATE_TRY(hipMalloc((void**)&h->weight, nvox * sizeof(float)));
  CREATE_TRY(hipMalloc((void**)&h->kfid, nvox * sizeof(uint32_t)));
  CREATE_TRY(hipMalloc((void**)&h->rgbw, nvox * sizeof(uint32_t)));
  CREATE_TRY(hipMalloc((void**)&h->d_ctr, sizeof(Counters)));
  CREATE_TRY(hipHostMalloc((void**)&h->h_ctr, sizeof(Counters), hipHostMallocCoherent));   // (read behind a polled word: wait_published)
  CREATE_TRY(hipMalloc((void**)&h->d_wctr, 2 * sizeof(WalkCounters)));
  CREATE_TRY(hipHostMalloc((void**)&h->h_wctr, 2 * sizeof(WalkCounters), hipHostMallocCoherent));
  CREATE_TRY(hipHostMalloc((void**)&h->h_seq, 64, hipHostMallocCoherent));
  h->h_seq[0] = 0u;
  {
    // Fixed-point scales of the order-free accumulators: a tile adds at most kWalkRays terms per voxel,
    // |w_u u| < weight / 2 and w_u <= weight / (2 diag); the largest powers of two that keep a tile's
    // sums inside 31 bits (one bit of headroom).
    const double wu_max = (double)p->weight / (2.0 * (double)P.diag), wuu_max = 0.5 * (double)p->weight;
    h->scale_u = (float)std::exp2(std::floor(std::log2(1073741824.0 / (kWalkRays * wuu_max))));
    h->scale_w = (float)std::exp2(std::floor(std::log2(1073741824.0 / (kWalkRays * wu_max))));
  }
  {
    // The side stream carries a long call's colour chain — the longer of the two branches behind the walk, a row of short
    // kernels — beside the apply stage's thousands of workgroups on the caller's stream: at the highest priority its
    // workgroups are dispatched ahead of the apply stage's queue instead of behind it.
    int least = 0, greatest = 0;
    CREATE_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    CREATE_TRY(hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, greatest));
  }
  CREATE_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
  CREATE_TRY(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
  CREATE_TRY(hipEventCreateWithFlags(&h->ev_seg, hipEventDisableTiming));
  CREATE_TRY(hipEventCreateWithFlags(&h->ev_zero, hipEventDisableTiming));
#undef CREATE_TRY
  *out = h;
  int rc = plvs_hip_tsdf_chisel_clear(h);
  if (rc != PLVS_OK) {
    plvs_hip_tsdf_chisel_destroy(h);
    *out = nullptr;
  }
  return rc;
}

int plvs_hip_tsdf_chisel_destroy(plvs_tsdf_chisel* h) {
  if (!h) return PLVS_OK;
  if (h->ext != nullptr && h->ext_free != nullptr) h->ext_free(h->ext);
  deform_state_free(h);
  (void)hipFree(h->dir.keys);
  (void)hipFree(h->dir.slots);
  (void)hipFree(h->dir.slot_ids);
  (void)hipFree(h->sdf);
  (void)hipFree(h->weight);
  (void)hipFree(h->kfid);
  (void)hipFree(h->rgbw);
  (void)hipFree(h->d_ctr);
  if (h->h_ctr) (void)hipHostFree(h->h_ctr);
  (void)hipFree(h->d_wctr);
  if (h->h_wctr) (void)hipHostFree(h->h_wctr);
  if (h->h_seq) (void)hipHostFree(h->h_seq);
  if (h->h_offsets) (void)hipHostFree(h->h_offsets);
  (void)hipFree(h->gdir.keys);
  (void)hipFree(h->gdir.slots);
  (void)hipFree(h->miss_keys);
  (void)hipFree(h->miss_ids);
  (void)hipFree(h->miss_count);
  (void)hipFree(h->xdir.keys);
  (void)hipFree(h->xdir.slots);
  (void)hipFree(h->xdir.slot_ids);
  (void)hipFree(h->d_xcount);
  (void)hipFree(h->x_sat);
  if (h->h_sh_counts) (void)hipHostFree(h->h_sh_counts);
  if (h->h_sh_ctl) (void)hipHostFree(h->h_sh_ctl);
  if (h->h_sh_off) (void)hipHostFree(h->h_sh_off);
  h->q_xyz.release(); h->q_rgb.release(); h->q_kfid.release();
  h->w_rec.release(); h->w_seg.release(); h->w_sorted_seg.release(); h->w_seg_ticket.release(); h->w_chunk_nseg.release();
  h->w_chunk_off.release(); h->w_chunk_fill.release(); h->w_active_off.release(); h->w_masks.release();
  h->w_dummy.release(); h->w_runkey.release(); h->w_run_cnt.release(); h->w_run_off.release(); h->w_val0.release();
  h->w_val1.release(); h->w_seg_cnt.release(); h->w_tile_visits.release(); h->w_deferred.release(); h->w_part_off.release(); h->w_multi_idx.release();
  h->pa_wuu.release(); h->pa_w.release(); h->pa_last.release(); h->pa_cnt.release(); h->pa_done.release();
  h->sh_nrec.release(); h->sh_owner.release(); h->halo_row.release();
  h->sh_ctl.release(); h->sh_seg_reg.release(); h->sh_rec_reg.release(); h->sh_src_off.release(); h->sh_slot_owner.release(); h->sh_run_ctr.release(); h->sh_vkey.release(); h->sh_sat.release(); h->sh_wait.release(); h->sh_run_first.release();
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->ev_seg) (void)hipEventDestroy(h->ev_seg);
  if (h->ev_zero) (void)hipEventDestroy(h->ev_zero);
  h->w_rseg.release(); h->w_rpre.release(); h->w_run_matrix.release(); h->w_active_idx.release(); h->w_item_base.release();
  h->w_item_cnt.release(); h->w_item_part0.release(); h->w_part_item.release(); h->w_phist.release();
  h->w_row_heads.release(); h->w_row_tot.release();
  if (h->side) (void)hipStreamDestroy(h->side);
  for (int i = 0; i <= kNumStages; ++i)
    if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
  h->counts.release();
  h->rec.release(); h->rec_t.release(); h->recc_t.release();
  h->dkey0.release(); h->dkey1.release(); h->didx0.release(); h->didx1.release();
  h->last_pt.release(); h->run_cnt.release(); h->run_dst.release();
  h->tile_first.release(); h->block_first.release(); h->tile_state.release();
  h->heads.release(); h->updated.release(); h->scratch.release(); h->poses.release();
  h->offsets.release(); h->st_xyz.release(); h->st_Twc.release(); h->st_nrm.release(); h->st_rgb.release();
  h->st_kfid.release();
  h->st_pos.release(); h->st_scan.release(); h->st_off.release();
  delete h;
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_clear(plvs_tsdf_chisel* h) {
  if (h) {   // (queued clouds belong to the map that is dropped)
    h->q_offsets.clear();
    h->q_Twc.clear();
  }
  PLVS_REQUIRE(h, "null handle");
  {
    int rc = halo_drop(h, nullptr);
    if (rc != PLVS_OK) return rc;
  }
  {
    int rc = shard_state_clear(h);   // (the walk directory of the ray-sharded integrate, if in use)
    if (rc != PLVS_OK) return rc;
  }
  const size_t cap = (size_t)h->dir.mask + 1;
  const size_t nvox = (size_t)h->prm.max_chunks * kChunkVox;
  PLVS_HIP_TRY(hipMemset(h->dir.keys, 0xFF, cap * sizeof(unsigned long long)));
  PLVS_HIP_TRY(hipMemset(h->dir.slots, 0xFF, cap * sizeof(int32_t)));
  PLVS_HIP_TRY(hipMemset(h->weight, 0, nvox * sizeof(float)));
  PLVS_HIP_TRY(hipMemset(h->kfid, 0, nvox * sizeof(uint32_t)));
  PLVS_HIP_TRY(hipMemset(h->rgbw, 0, nvox * sizeof(uint32_t)));
  PLVS_HIP_TRY(hipMemset(h->d_ctr, 0, sizeof(Counters)));
  hipLaunchKernelGGL(pool_init, dim3(2048), dim3(256), 0, nullptr, h->sdf, nvox);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(hipDeviceSynchronize());
  h->num_chunks = 0;
  h->walk.small_runs_known = false;   // (the first call on the empty map reads its own run count)
  h->poisoned = false;
  h->stats = plvs_tsdf_stats{};
  h->last_updated = 0;
  deform_state_clear(h);
  return PLVS_OK;
}

}  // extern "C"

// One batch of point clouds into the map: the call checked, then the pipeline of the handle's mode.
// d_normals != nullptr: the world-cloud-with-normals flavour (Chisel::IntegrateWorldPointCloudWithNormals), always
// through the ordered pipeline.
static int integrate_batch_core(plvs_tsdf_chisel* h, const float* d_xyz, const uint8_t* d_rgb, const uint32_t* d_kfid,
                                const int32_t* offsets, int nclouds, const float* d_Twc, void* stream,
                                const float* d_normals) {
  PLVS_REQUIRE(h, "null handle");
  PLVS_REQUIRE(!h->poisoned, "handle is in a failed state (clear it)");
  PLVS_REQUIRE(offsets && nclouds >= 0, "bad offsets");
  hipStream_t s = static_cast<hipStream_t>(stream);
  h->stats = plvs_tsdf_stats{};
  h->last_updated = 0;
  int n = 0;
  int rc = check_offsets(offsets, nclouds, &n);
  if (rc != PLVS_OK || nclouds == 0) return rc;
  h->stats.points = n;
  if (n == 0) return PLVS_OK;
  PLVS_REQUIRE(d_xyz && d_rgb && d_Twc, "null device pointer");
  if ((rc = halo_drop(h, s)) != PLVS_OK) return rc;   // new chunks go into the pool slots a meshing halo may still occupy
  PLVS_HIP_TRY(h->offsets.reserve(2 * ((size_t)nclouds + 1)));
  PLVS_HIP_TRY(h->poses.reserve((size_t)nclouds));
  if (h->prm.order_free != 0 && d_normals == nullptr) return integrate_walk_acc(h, d_xyz, d_rgb, d_kfid, n, nclouds, offsets, d_Twc, s);
  return integrate_ordered(h, d_xyz, d_rgb, d_kfid, n, nclouds, offsets, d_Twc, s, d_normals);
}

static int integrate_batch_impl(plvs_tsdf_chisel* h, const float* d_xyz, const uint8_t* d_rgb, const uint32_t* d_kfid,
                                const int32_t* offsets, int nclouds, const float* d_Twc, void* stream,
                                const float* d_normals) {
  PLVS_REQUIRE(h, "null handle");
  // a map with deform enabled keeps the reference's chunk-map order: the call's visits are replayed first
  const bool track = h->dfm != nullptr && !h->poisoned && offsets && nclouds >= 1 && offsets[nclouds] - offsets[0] > 0 && d_xyz &&
                     d_Twc;
  if (track) {
    int rc = halo_drop(h, static_cast<hipStream_t>(stream));
    if (rc == PLVS_OK) rc = deform_track_begin(h, d_xyz, d_normals, offsets[nclouds] - offsets[0], nclouds, d_Twc, static_cast<hipStream_t>(stream));
    if (rc != PLVS_OK) return rc;
  }
  int rc = integrate_batch_core(h, d_xyz, d_rgb, d_kfid, offsets, nclouds, d_Twc, stream, d_normals);
  if (track && rc == PLVS_OK) rc = deform_track_end(h, static_cast<hipStream_t>(stream));
  return rc;
}

extern "C" {

int plvs_hip_tsdf_chisel_integrate_batch_dev(plvs_tsdf_chisel* h, const float* d_xyz,
                                             const uint8_t* d_rgb, const uint32_t* d_kfid,
                                             const int32_t* offsets, int nclouds,
                                             const float* d_Twc, void* stream) {
  PLVS_FLUSH_QUEUE(h);
  return integrate_batch_impl(h, d_xyz, d_rgb, d_kfid, offsets, nclouds, d_Twc, stream, nullptr);
}

// ---- depth images straight into the map (round 5): GeneratePointCloudInCameraFrameBGRA + InsertCloud in one call.
// Order-free handles walk 32 x 16 blocks of grid pixels (GridSrc, tsdf_walk.hpp): the cloud is never written.  Ordered
// handles (and sharded ones) build the reference's clouds in scratch memory — raster-order compaction of the valid grid
// pixels — and take the ordinary batch path: bit for bit plvs_hip_cloudgen_generate_dev + integrate_batch_dev.
int plvs_hip_tsdf_chisel_integrate_depth_batch_dev(plvs_tsdf_chisel* h, const plvs_depth_batch* in, int nclouds,
                                                   const float* d_Twc, void* stream) {
  PLVS_FLUSH_QUEUE(h);
  PLVS_REQUIRE(h && in, "null argument");
  PLVS_REQUIRE(!h->poisoned, "handle is in a failed state (clear it)");
  PLVS_REQUIRE(nclouds >= 0, "bad image count");
  h->stats = plvs_tsdf_stats{};
  h->last_updated = 0;
  if (nclouds == 0) return PLVS_OK;
  PLVS_REQUIRE(in->d_depth && in->d_bgr && in->d_grid_points && d_Twc, "null device pointer");
  PLVS_REQUIRE(in->width > 0 && in->height > 0 && in->step > 0, "image size / step");
  PLVS_REQUIRE(in->depth_pitch >= in->width && in->bgr_pitch >= 3 * in->width, "row pitch smaller than a row");
  PLVS_REQUIRE(in->depth_image_stride >= (size_t)in->depth_pitch * (size_t)(in->height - 1) + (size_t)in->width &&
               in->bgr_image_stride >= (size_t)in->bgr_pitch * (size_t)(in->height - 1) + 3 * (size_t)in->width,
               "image stride smaller than an image");
  hipStream_t s = static_cast<hipStream_t>(stream);
  GridSrc g{};
  g.depth = in->d_depth;
  g.cam = in->d_grid_points;
  g.image_stride = in->depth_image_stride;
  g.pitch = (uint32_t)in->depth_pitch;
  g.step = (uint32_t)in->step;
  g.gw = (uint32_t)((in->width + in->step - 1) / in->step);
  g.gh = (uint32_t)((in->height + in->step - 1) / in->step);
  g.ntx = (g.gw + kGridTileW - 1) / kGridTileW;
  g.nty = (g.gh + kGridTileH - 1) / kGridTileH;
  g.inv_ntx = 1.0f / (float)g.ntx;
  g.inv_nty = 1.0f / (float)g.nty;
  g.key_bits = 1;
  while ((1ull << g.key_bits) < (unsigned long long)g.gw * g.gh) ++g.key_bits;
  g.min_depth = in->min_depth;
  g.max_depth = in->max_depth;
  g.bgr_image_stride = in->bgr_image_stride;
  g.bgr_pitch = (uint32_t)in->bgr_pitch;
  PLVS_REQUIRE(g.key_bits < 31 && (unsigned long long)nclouds <= (1ull << (32 - g.key_bits)),
               "too many images in one call for the order keys (split the batch)");
  const size_t ngrid = (size_t)g.gw * g.gh;
  h->stats.points = 0;
  {
    int rc = halo_drop(h, s);   // new chunks go into the pool slots a meshing halo may still occupy
    if (rc != PLVS_OK) return rc;
  }
  const bool walk2d = h->prm.order_free != 0 && std::max(1, h->prm.shard_count) == 1 && h->dfm == nullptr;
  if (walk2d) {
    std::vector<int32_t> zeros((size_t)nclouds + 1, 0);
    PLVS_HIP_TRY(h->offsets.reserve(2 * ((size_t)nclouds + 1)));
    PLVS_HIP_TRY(h->poses.reserve((size_t)nclouds));
    return integrate_walk_acc(h, nullptr, in->d_bgr, in->d_kfid, 0, nclouds, zeros.data(), d_Twc, s, &g);
  }
  // ---- the reference's clouds, in scratch memory
  const size_t cells = ngrid * (size_t)nclouds;
  PLVS_REQUIRE(cells < 0x7FFFFFFFull, "too many grid pixels in one call (split the batch)");
  // (the scratch of this path lives with the handle: allocated on the handle's device, released by destroy)
  plvs::DevBuf<uint32_t>&pos = h->st_pos, &scan_scratch = h->st_scan, &d_off = h->st_off;
  PLVS_HIP_TRY(pos.reserve(cells + 1));
  PLVS_HIP_TRY(scan_scratch.reserve(scan_scratch_words(cells)));
  PLVS_HIP_TRY(d_off.reserve((size_t)nclouds + 1));
  PLVS_HIP_TRY(h->st_xyz.reserve(cells * 3));
  PLVS_HIP_TRY(h->st_rgb.reserve(cells * 3));
  PLVS_HIP_TRY(h->st_kfid.reserve(cells));
  hipLaunchKernelGGL(grid_cloud_mark, dim3(ceil_div(cells, 256)), dim3(256), 0, s, g, nclouds, pos.p);
  PLVS_HIP_TRY(exclusive_scan_u32(pos.p, pos.p, cells, pos.p + cells, scan_scratch.p, s));
  hipLaunchKernelGGL(grid_cloud_emit, dim3(ceil_div(cells + 1, 256)), dim3(256), 0, s, g, nclouds, (const uint32_t*)pos.p, in->d_bgr,
                     in->d_kfid, h->st_xyz.p, h->st_rgb.p, h->st_kfid.p, d_off.p);
  PLVS_KERNEL_CHECK();
  std::vector<int32_t> offsets((size_t)nclouds + 1);
  PLVS_HIP_TRY(hipMemcpyAsync(offsets.data(), d_off.p, ((size_t)nclouds + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  PLVS_HIP_TRY(hipStreamSynchronize(s));
  return integrate_batch_impl(h, h->st_xyz.p, h->st_rgb.p, in->d_kfid ? h->st_kfid.p : nullptr, offsets.data(), nclouds, d_Twc,
                              stream, nullptr);
}

int plvs_hip_tsdf_chisel_integrate_world_normals_dev(plvs_tsdf_chisel* h, const float* d_xyz, const uint8_t* d_rgb,
                                                     const uint32_t* d_kfid, const float* d_normals, int n,
                                                     const float* d_Twc, void* stream) {
  PLVS_FLUSH_QUEUE(h);
  PLVS_REQUIRE(h && n >= 0, "bad arguments");
  PLVS_REQUIRE(n == 0 || d_normals, "null normals");
  PLVS_REQUIRE(std::max(1, h->prm.shard_count) == 1 || h->prm.order_free == 0,
               "a ray-sharded (order_free) map takes the world cloud on the rank that owns each chunk: use an ordered sharded handle");
  const int32_t offsets[2] = {0, n};
  return integrate_batch_impl(h, d_xyz, d_rgb, d_kfid, offsets, 1, d_Twc, stream, d_normals);
}

int plvs_hip_tsdf_chisel_integrate_world_normals(plvs_tsdf_chisel* h, const float* xyz, const uint8_t* rgb,
                                                 const uint32_t* kfid, const float* normals, int n, const float* Twc) {
  PLVS_FLUSH_QUEUE(h);
  PLVS_REQUIRE(h, "null handle");
  PLVS_REQUIRE(n >= 0 && Twc, "bad arguments");
  h->stats = plvs_tsdf_stats{};
  h->last_updated = 0;
  if (n == 0) return PLVS_OK;
  PLVS_REQUIRE(xyz && rgb && normals, "null input");
  PLVS_HIP_TRY(h->st_xyz.reserve((size_t)n * 3));
  PLVS_HIP_TRY(h->st_rgb.reserve((size_t)n * 3));
  PLVS_HIP_TRY(h->st_Twc.reserve(12));
  PLVS_HIP_TRY(h->st_nrm.reserve((size_t)n * 3));
  if (kfid) PLVS_HIP_TRY(h->st_kfid.reserve((size_t)n));
  PLVS_HIP_TRY(hipMemcpy(h->st_xyz.p, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->st_rgb.p, rgb, (size_t)n * 3, hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->st_nrm.p, normals, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->st_Twc.p, Twc, 12 * sizeof(float), hipMemcpyHostToDevice));
  if (kfid) PLVS_HIP_TRY(hipMemcpy(h->st_kfid.p, kfid, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
  const int rc = plvs_hip_tsdf_chisel_integrate_world_normals_dev(h, h->st_xyz.p, h->st_rgb.p, kfid ? h->st_kfid.p : nullptr,
                                                                  h->st_nrm.p, n, h->st_Twc.p, nullptr);
  (void)hipDeviceSynchronize();
  return rc;
}

// ---- queued integration.  PLVS hands a key frame's cloud over with InsertCloud and reads the map only in UpdateMap, after
// at most five of them (src/PointCloudMapping.cc:540-552, 594-598).  _queue uploads the cloud and returns; _flush
// integrates everything queued in ONE call of the batch pipeline — the same result as integrating the clouds one by one
// (bit for bit in the ordered mode: the batch pipeline applies every update in point order across the clouds; within the
// stated tolerance in the order-free mode, where a voxel takes one update per CALL) at a fraction of the per-call
// launch chain.  Every entry point that reads or changes the map flushes first.
int plvs_hip_tsdf_chisel_queue(plvs_tsdf_chisel* h, const float* xyz, const uint8_t* rgb, const uint32_t* kfid, int n,
                               const float* Twc) {
  PLVS_REQUIRE(h, "null handle");
  PLVS_REQUIRE(n >= 0 && Twc, "bad arguments");
  if (n == 0) return PLVS_OK;
  PLVS_REQUIRE(xyz && rgb, "null cloud pointer");
  const bool first = h->q_offsets.empty();
  PLVS_REQUIRE(first || h->q_kfid_given == (kfid != nullptr), "queued clouds must all carry key-frame ids, or none");
  const size_t at = first ? 0 : (size_t)h->q_offsets.back();
  PLVS_REQUIRE(at + (size_t)n < 0x7FFFFFFFull, "too many queued points");
  PLVS_HIP_TRY(grow_keep(h->q_xyz, 3 * at, 3 * (at + (size_t)n)));
  PLVS_HIP_TRY(grow_keep(h->q_rgb, 3 * at, 3 * (at + (size_t)n)));
  PLVS_HIP_TRY(hipMemcpy(h->q_xyz.p + 3 * at, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->q_rgb.p + 3 * at, rgb, (size_t)n * 3, hipMemcpyHostToDevice));
  if (kfid) {
    PLVS_HIP_TRY(grow_keep(h->q_kfid, at, at + (size_t)n));
    PLVS_HIP_TRY(hipMemcpy(h->q_kfid.p + at, kfid, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  if (first) h->q_offsets.push_back(0);
  h->q_kfid_given = kfid != nullptr;
  h->q_offsets.push_back((int32_t)(at + (size_t)n));
  h->q_Twc.insert(h->q_Twc.end(), Twc, Twc + 12);
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_queued(plvs_tsdf_chisel* h, int* nclouds) {
  PLVS_REQUIRE(h && nclouds, "null argument");
  *nclouds = h->q_offsets.empty() ? 0 : (int)h->q_offsets.size() - 1;
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_flush(plvs_tsdf_chisel* h) {
  PLVS_REQUIRE(h, "null handle");
  if (h->q_offsets.empty()) return PLVS_OK;
  const int nclouds = (int)h->q_offsets.size() - 1;
  std::vector<int32_t> offsets;
  std::vector<float> Twc;
  offsets.swap(h->q_offsets);   // (the queue is empty from here on: the integrate below flushes nothing)
  Twc.swap(h->q_Twc);
  PLVS_HIP_TRY(h->st_Twc.reserve((size_t)12 * nclouds));
  PLVS_HIP_TRY(hipMemcpy(h->st_Twc.p, Twc.data(), (size_t)12 * nclouds * sizeof(float), hipMemcpyHostToDevice));
  int rc = plvs_hip_tsdf_chisel_integrate_batch_dev(h, h->q_xyz.p, h->q_rgb.p, h->q_kfid_given ? h->q_kfid.p : nullptr,
                                                    offsets.data(), nclouds, h->st_Twc.p, nullptr);
  if (rc != PLVS_OK) {
    // The queue was taken before the batch ran (a reader that flushes must not flush again from inside it): its clouds are
    // gone.  Say so, and how many — the error surfaces from whichever call triggered the flush, possibly a reader.
    char own[400];
    snprintf(own, sizeof own, "%s", plvs::last_error_buf());
    plvs::set_error("%s — raised by the flush of %d queued key-frame cloud%s (plvs_hip_tsdf_chisel_queue): NONE of them was "
                    "integrated and they are dropped; queue them again after clearing / enlarging the map", own, nclouds,
                    nclouds == 1 ? "" : "s");
    return rc;
  }
  PLVS_HIP_TRY(hipDeviceSynchronize());
  return PLVS_OK;
}
int plvs_hip_tsdf_chisel_integrate(plvs_tsdf_chisel* h, const float* xyz, const uint8_t* rgb,
                                   const uint32_t* kfid, int n, const float* Twc) {
  PLVS_REQUIRE(h, "null handle");
  PLVS_REQUIRE(n >= 0 && Twc, "bad arguments");
  PLVS_FLUSH_QUEUE(h);
  if (n == 0) {
    h->stats = plvs_tsdf_stats{};
    h->last_updated = 0;
    return PLVS_OK;
  }
  PLVS_REQUIRE(xyz && rgb, "null cloud pointer");
  PLVS_HIP_TRY(h->st_xyz.reserve((size_t)n * 3));
  PLVS_HIP_TRY(h->st_rgb.reserve((size_t)n * 3));
  PLVS_HIP_TRY(h->st_Twc.reserve(12));
  PLVS_HIP_TRY(hipMemcpy(h->st_xyz.p, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->st_rgb.p, rgb, (size_t)n * 3, hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->st_Twc.p, Twc, 12 * sizeof(float), hipMemcpyHostToDevice));
  const uint32_t* dk = nullptr;
  if (kfid) {
    PLVS_HIP_TRY(h->st_kfid.reserve((size_t)n));
    PLVS_HIP_TRY(hipMemcpy(h->st_kfid.p, kfid, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    dk = h->st_kfid.p;
  }
  const int32_t offsets[2] = {0, n};
  int rc = plvs_hip_tsdf_chisel_integrate_batch_dev(h, h->st_xyz.p, h->st_rgb.p, dk, offsets, 1,
                                                    h->st_Twc.p, nullptr);
  if (rc != PLVS_OK) return rc;
  PLVS_HIP_TRY(hipDeviceSynchronize());
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_set_apply_parts(plvs_tsdf_chisel* h, int part_segments, int min_segments) {
  PLVS_REQUIRE(h && part_segments >= 1 && min_segments >= 1, "bad argument");
  h->part_segs = (uint32_t)part_segments;
  h->part_min = (uint32_t)min_segments;
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_set_profiling(plvs_tsdf_chisel* h, int enable) {
  PLVS_REQUIRE(h, "null handle");
  if (enable && !h->ev[0])
    for (int i = 0; i <= kNumStages; ++i) PLVS_HIP_TRY(hipEventCreate(&h->ev[i]));
  h->profiling = enable != 0;
  for (int i = 0; i < kNumStages; ++i) h->stage_ms[i] = 0.0;
  h->prof_calls = 0;
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_stage_ms(plvs_tsdf_chisel* h, double* ms, int cap, int* nstages,
                                  int64_t* calls) {
  PLVS_REQUIRE(h && nstages, "null argument");
  *nstages = h->stage_set == 1 ? kWalkStages : kNumStages;
  if (calls) *calls = h->prof_calls;
  for (int i = 0; i < kNumStages && i < cap; ++i) ms[i] = h->stage_ms[i];
  return PLVS_OK;
}

const char* plvs_hip_tsdf_chisel_stage_name(int i) {
  return (i >= 0 && i < kNumStages) ? kStageNames[i] : "";
}

const char* plvs_hip_tsdf_chisel_stage_name_of(plvs_tsdf_chisel* h, int i) {
  if (h == nullptr || i < 0) return "";
  if (h->stage_set == 1) return i < kWalkStages ? kWalkStageNames[i] : "";
  return i < kNumStages ? kStageNames[i] : "";
}

__global__ void gather_slot_ids(const uint32_t* __restrict__ slots, int n,
                                const int32_t* __restrict__ slot_ids, int32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const uint32_t s = slots[i];
    out[3 * i] = slot_ids[3 * s];
    out[3 * i + 1] = slot_ids[3 * s + 1];
    out[3 * i + 2] = slot_ids[3 * s + 2];
  }
}

int plvs_hip_tsdf_chisel_updated_chunk_ids_dev(plvs_tsdf_chisel* h, int32_t* d_ids_xyz, int cap,
                                               int* n, void* stream) {
  PLVS_FLUSH_QUEUE(h);
  PLVS_REQUIRE(h && n, "null argument");
  *n = (int)h->last_updated;
  const int m = (int)h->last_updated < cap ? (int)h->last_updated : cap;
  if (m <= 0) return PLVS_OK;
  PLVS_REQUIRE(d_ids_xyz, "null output");
  hipLaunchKernelGGL(gather_slot_ids, dim3(ceil_div((size_t)m, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), h->updated.p, m, h->dir.slot_ids, d_ids_xyz);
  PLVS_KERNEL_CHECK();
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_last_stats(plvs_tsdf_chisel* h, plvs_tsdf_stats* s) {
  PLVS_FLUSH_QUEUE(h);
  PLVS_REQUIRE(h && s, "null argument");
  *s = h->stats;
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_num_chunks(plvs_tsdf_chisel* h, int* n) {
  PLVS_FLUSH_QUEUE(h);
  PLVS_REQUIRE(h && n, "null argument");
  *n = h->num_chunks;
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_chunk_ids(plvs_tsdf_chisel* h, int32_t* ids_xyz, int cap, int* n) {
  PLVS_FLUSH_QUEUE(h);
  PLVS_REQUIRE(h && n, "null argument");
  *n = h->num_chunks;
  const int m = h->num_chunks < cap ? h->num_chunks : cap;
  if (m > 0) {
    PLVS_REQUIRE(ids_xyz, "null output");
    PLVS_HIP_TRY(hipMemcpy(ids_xyz, h->dir.slot_ids, (size_t)m * 3 * sizeof(int32_t),
                           hipMemcpyDeviceToHost));
  }
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_updated_chunk_ids(plvs_tsdf_chisel* h, int32_t* ids_xyz, int cap, int* n) {
  PLVS_FLUSH_QUEUE(h);
  PLVS_REQUIRE(h && n, "null argument");
  *n = (int)h->last_updated;
  const int m = (int)h->last_updated < cap ? (int)h->last_updated : cap;
  if (m <= 0) return PLVS_OK;
  PLVS_REQUIRE(ids_xyz, "null output");
  // small lists: resolve slot -> id on the host
  uint32_t* slots = new uint32_t[h->last_updated];
  int32_t* all = new int32_t[(size_t)h->num_chunks * 3];
  hipError_t e1 = hipMemcpy(slots, h->updated.p, (size_t)h->last_updated * sizeof(uint32_t),
                            hipMemcpyDeviceToHost);
  hipError_t e2 = hipMemcpy(all, h->dir.slot_ids, (size_t)h->num_chunks * 3 * sizeof(int32_t),
                            hipMemcpyDeviceToHost);
  if (e1 == hipSuccess && e2 == hipSuccess)
    for (int i = 0; i < m; ++i) memcpy(ids_xyz + 3 * i, all + 3 * (size_t)slots[i], 3 * sizeof(int32_t));
  delete[] slots;
  delete[] all;
  PLVS_HIP_TRY(e1);
  PLVS_HIP_TRY(e2);
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_download_chunk(plvs_tsdf_chisel* h, int cx, int cy, int cz, float* sdf,
                                        float* weight, uint32_t* kfid, uint32_t* rgbw) {
  PLVS_FLUSH_QUEUE(h);
  PLVS_REQUIRE(h && sdf && weight && kfid && rgbw, "null argument");
  // linear search of the (host-copied) slot table; a download is a debug /
  // meshing hand-off, not part of the integrate path.
  int32_t* all = new int32_t[(size_t)(h->num_chunks > 0 ? h->num_chunks : 1) * 3];
  hipError_t e = hipSuccess;
  if (h->num_chunks > 0)
    e = hipMemcpy(all, h->dir.slot_ids, (size_t)h->num_chunks * 3 * sizeof(int32_t),
                  hipMemcpyDeviceToHost);
  int slot = -1;
  if (e == hipSuccess)
    for (int i = 0; i < h->num_chunks; ++i)
      if (all[3 * i] == cx && all[3 * i + 1] == cy && all[3 * i + 2] == cz) { slot = i; break; }
  delete[] all;
  PLVS_HIP_TRY(e);
  if (slot < 0) {
    plvs::set_error("chunk (%d,%d,%d) does not exist", cx, cy, cz);
    return PLVS_ERR_INVALID_ARG;
  }
  const size_t off = (size_t)slot * kChunkVox;
  PLVS_HIP_TRY(hipMemcpy(sdf, h->sdf + off, kChunkVox * sizeof(float), hipMemcpyDeviceToHost));
  PLVS_HIP_TRY(hipMemcpy(weight, h->weight + off, kChunkVox * sizeof(float), hipMemcpyDeviceToHost));
  PLVS_HIP_TRY(hipMemcpy(kfid, h->kfid + off, kChunkVox * sizeof(uint32_t), hipMemcpyDeviceToHost));
  PLVS_HIP_TRY(hipMemcpy(rgbw, h->rgbw + off, kChunkVox * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return PLVS_OK;
}

}  // extern "C"

namespace plvs {
namespace tsdf {

bool chisel_map_view(plvs_tsdf_chisel* h, ChiselMapView* v) {
  if (h == nullptr || v == nullptr || h->poisoned) return false;
  v->resolution = h->P.resolution;
  v->dir = h->dir;
  v->sdf = h->sdf;
  v->weight = h->weight;
  v->kfid = h->kfid;
  v->rgbw = h->rgbw;
  v->num_chunks = h->num_chunks;
  v->shard_count = h->P.shard_count;
  v->shard_rank = h->P.shard_rank;
  v->ext = &h->ext;
  v->ext_free = &h->ext_free;
  if (h->P.shard_count > 1) {
    if (h->miss_keys == nullptr) {
      // every chunk of the whole map could be asked for, and many ids that exist nowhere (InterpolateColor's look-ups at
      // voxel indices used as metres reach ~20 chunk widths: thousands of distinct ids per call): at least 2^18 entries
      const size_t want = std::max<size_t>(std::min<size_t>((size_t)h->prm.max_chunks * (size_t)h->P.shard_count, (size_t)1 << 22),
                                           (size_t)1 << 18);
      size_t cap = 1024;
      while (cap < 2 * want) cap <<= 1;
      if (hipMalloc(&h->miss_keys, cap * sizeof(unsigned long long)) != hipSuccess) return false;
      if (hipMalloc(&h->miss_ids, want * 3 * sizeof(int32_t)) != hipSuccess) return false;
      if (hipMalloc(&h->miss_count, sizeof(uint32_t)) != hipSuccess) return false;
      h->miss_cap = (uint32_t)want;
      h->miss_mask = (uint32_t)(cap - 1);
    }
    if (hipMemsetAsync(h->miss_keys, 0xFF, ((size_t)h->miss_mask + 1) * sizeof(unsigned long long), nullptr) != hipSuccess) return false;
    if (hipMemsetAsync(h->miss_count, 0, sizeof(uint32_t), nullptr) != hipSuccess) return false;
    v->ghost = h->gdir;
    v->miss_keys = h->miss_keys;
    v->miss_mask = h->miss_mask;
    v->miss_ids = h->miss_ids;
    v->miss_count = h->miss_count;
    v->miss_cap = h->miss_cap;
  }
  return true;
}

}  // namespace tsdf
}  // namespace plvs

// One chunk id -> its pool slot, created if absent (plvs_hip_tsdf_chisel_upload_chunk).
__global__ void chunk_slot_of(Directory dir, int x, int y, int z, int32_t* __restrict__ num_chunks, uint32_t* __restrict__ err,
                              int32_t* __restrict__ slot_out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *slot_out = dir_find_or_insert(dir, x, y, z, num_chunks, err);
}

extern "C" {

// Creates or REPLACES one chunk with the given voxel planes (host, 4096 each, id = (z * 16 + y) * 16 + x): the way a
// volume saved with download_chunk comes back, and what lets tests put analytic distance fields on the device.
int plvs_hip_tsdf_chisel_upload_chunk(plvs_tsdf_chisel* h, int cx, int cy, int cz, const float* sdf, const float* weight,
                                      const uint32_t* kfid, const uint32_t* rgbw) {
  PLVS_FLUSH_QUEUE(h);
  PLVS_REQUIRE(h && sdf && weight && kfid && rgbw, "null argument");
  PLVS_REQUIRE(!h->poisoned, "handle is in a failed state (clear it)");
  if (std::max(1, h->prm.shard_count) > 1)
    PLVS_REQUIRE(shard_of(chunk_hash(cx, cy, cz), h->prm.shard_count) == h->prm.shard_rank, "the chunk belongs to another rank");
  int rc = halo_drop(h, nullptr);
  if (rc != PLVS_OK) return rc;
  PLVS_HIP_TRY(hipMemset(&h->d_ctr->err, 0, sizeof(uint32_t)));
  int32_t* d_slot = reinterpret_cast<int32_t*>(&h->d_ctr->total_visits);   // (a counter no call is using now)
  hipLaunchKernelGGL(chunk_slot_of, dim3(1), dim3(64), 0, nullptr, h->dir, cx, cy, cz, &h->d_ctr->num_chunks, &h->d_ctr->err,
                     d_slot);
  PLVS_KERNEL_CHECK();
  rc = read_counters(h, nullptr);
  if (rc != PLVS_OK) return rc;
  if (h->h_ctr->err) {
    h->poisoned = true;
    plvs::set_error("upload_chunk: %s", (h->h_ctr->err & kErrPoolFull) ? "chunk pool full (raise max_chunks)" : "chunk id out of range");
    return PLVS_ERR_CAPACITY;
  }
  const int slot = (int)h->h_ctr->total_visits;
  h->num_chunks = h->h_ctr->num_chunks;
  if (h->dfm) deform_note_created(h, cx, cy, cz);
  const size_t off = (size_t)slot * kChunkVox;
  PLVS_HIP_TRY(hipMemcpy(h->sdf + off, sdf, kChunkVox * sizeof(float), hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->weight + off, weight, kChunkVox * sizeof(float), hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->kfid + off, kfid, kChunkVox * sizeof(uint32_t), hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->rgbw + off, rgbw, kChunkVox * sizeof(uint32_t), hipMemcpyHostToDevice));
  return PLVS_OK;
}

}  // extern "C"
