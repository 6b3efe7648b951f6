// Host side of the voxblox back end's ordered pipeline (kernels: tsdf_voxblox_kernels.hpp): head of a call -> count pass +
// scan -> fill pass -> tail (stable radix sort by voxel, expansion, fold, counters, stats).  vb_integrate_impl is that
// sequence for the four flavours of the ray passes; the ray-sharded integrate (tsdf_voxblox_shard.hpp) fills the records
// its own way between the same head and the same tail.  Also here: staging of a host cloud and the empty scan of the host
// flavours.
#pragma once
#include <algorithm>
#include <vector>

#include "tsdf_voxblox_kernels.hpp"
#include "tsdf_voxblox_halo.hpp"
#include "tsdf_voxblox_fast.hpp"

// Blocks a world cloud left waiting (slots [lo, hi)) have just joined the layer with their Block::updated() flags set
// (integrateWorlPointCloud marks them, tsdf_integrator.cc:76-80): they belong to this call's updated list even if this
// call's rays did not touch them.  Rare (once after a LoadMap): done on the host.
static int vb_publish_waiting(plvs_tsdf_voxblox* h, hipStream_t s, int published_lo, int published_hi) {
  if (published_hi <= published_lo) return PLVS_OK;
  std::vector<uint32_t> upd(h->last_updated);
  if (!upd.empty()) PLVS_HIP_TRY(hipMemcpyAsync(upd.data(), h->updated.p, upd.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PLVS_HIP_TRY(hipStreamSynchronize(s));
  std::vector<uint8_t> in((size_t)(published_hi - published_lo), 0);
  for (uint32_t v : upd)
    if ((int)v >= published_lo && (int)v < published_hi) in[(size_t)((int)v - published_lo)] = 1;
  for (int v = published_lo; v < published_hi; ++v)
    if (!in[(size_t)(v - published_lo)]) upd.push_back((uint32_t)v);
  std::sort(upd.begin(), upd.end());
  PLVS_HIP_TRY(h->upd_merge.reserve(upd.size() + 1));
  PLVS_HIP_TRY(hipMemcpy(h->upd_merge.p, upd.data(), upd.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  std::swap(h->updated.p, h->upd_merge.p);
  std::swap(h->updated.cap, h->upd_merge.cap);
  h->last_updated = (uint32_t)upd.size();
  h->stats.updated_chunks = (int32_t)upd.size();
  return PLVS_OK;
}

// A camera cloud, even an empty one, starts with updateLayerWithStoredBlocks (tsdf_integrator.cc:306 / :343): every waiting
// block joins the layer.
static int vb_publish_all(plvs_tsdf_voxblox* h, hipStream_t s) {
  const int lo = h->visible_blocks, hi = h->num_blocks;
  h->visible_blocks = h->num_blocks;
  return vb_publish_waiting(h, s, lo, hi);
}

// Head of a call: the cloud offsets on the device, the call's counters zero, the poses with their quaternions.
static int vb_call_head(plvs_tsdf_voxblox* h, const int32_t* offsets, int nclouds, const float* d_Twc, hipStream_t s) {
  PLVS_HIP_TRY(h->offsets.reserve((size_t)nclouds + 1));
  PLVS_HIP_TRY(hipMemcpyAsync(h->offsets.p, offsets, ((size_t)nclouds + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
  PLVS_HIP_TRY(hipMemsetAsync(&h->d_ctr->total_visits, 0, sizeof(uint32_t), s));
  PLVS_HIP_TRY(hipMemsetAsync(&h->d_ctr->err, 0, 4 * sizeof(uint32_t), s));
  PLVS_HIP_TRY(h->poses.reserve((size_t)nclouds));
  hipLaunchKernelGGL(vb_pose_prep, dim3(ceil_div((size_t)nclouds, 64)), dim3(64), 0, s, d_Twc, nclouds, h->poses.p);
  return PLVS_OK;
}

// The ray pass of a flavour over the call's n rays: the count pass (visits per ray into h->counts, new blocks into the
// directory) or, with the counts scanned, the fill pass (records into keys0 / seq0).
template <bool kFill>
static void vb_launch_ray_pass(plvs_tsdf_voxblox* h, hipStream_t s, int mode, const float* d_xyz, const float* d_aux,
                               const uint8_t* d_clr, int n, int nclouds) {
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(ceil_div((size_t)n, 256)), dim3(256), 0, s, h->P, d_xyz, d_aux, d_clr, n, h->offsets.p, nclouds,
                       h->poses.p, h->dir, h->d_ctr, h->counts.p, kFill ? h->keys0.p : (uint32_t*)nullptr,
                       kFill ? h->seq0.p : (uint32_t*)nullptr);
  };
  switch (mode) {
    case kWorld: launch(vb_ray_pass<kFill, kWorld>); break;
    case kMerged: launch(vb_ray_pass<kFill, kMerged>); break;
    case kFast: launch(vb_ray_pass<kFill, kFast>); break;
    default: launch(vb_ray_pass<kFill, kSimple>); break;
  }
}

// ... and the expansion of the V sorted records (a fast ray's record is a simple ray's: the mixed order, the point's weight).
static void vb_launch_expand(plvs_tsdf_voxblox* h, hipStream_t s, int mode, const uint32_t* keys, const uint32_t* seqs, uint32_t V,
                             const float* d_xyz, const float* d_aux, const uint32_t* d_col, int nclouds) {
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(ceil_div(V, kExpandThreads)), dim3(kExpandThreads), 0, s, h->P, keys, seqs, V, d_xyz, d_aux, d_col,
                       h->offsets.p, nclouds, h->poses.p, h->dir.slot_ids, h->rec.p, h->rec_c.p, h->heads.p, h->updated.p, h->d_ctr);
  };
  switch (mode) {
    case kWorld: launch(vb_expand<kWorld>); break;
    case kMerged: launch(vb_expand<kMerged>); break;
    default: launch(vb_expand<kSimple>); break;
  }
}

// The buffers of a call of V voxel visits (the updated list follows the number of blocks: the tail reserves it).
static int vb_reserve_visits(plvs_tsdf_voxblox* h, uint32_t V) {
  PLVS_HIP_TRY(h->keys0.reserve(V));
  PLVS_HIP_TRY(h->keys1.reserve(V));
  PLVS_HIP_TRY(h->seq0.reserve(V));
  PLVS_HIP_TRY(h->seq1.reserve(V));
  PLVS_HIP_TRY(h->heads.reserve(V));
  PLVS_HIP_TRY(h->rec.reserve(V));
  PLVS_HIP_TRY(h->rec_c.reserve(V));
  PLVS_HIP_TRY(h->scratch.reserve(radix_scratch_words(V)));
  return PLVS_OK;
}

// Tail of a call: the V records in keys0 / seq0 (voxel key, sequence number; h->num_blocks final) sorted by voxel, expanded
// to operands and folded into the map; then the counters, the call's stats and the blocks [published_lo, published_hi)
// that joined the layer with this call.  `call`: the entry point's name in messages.
static int vb_sort_and_fold(plvs_tsdf_voxblox* h, hipStream_t s, int mode, uint32_t V, const float* d_xyz, const float* d_aux,
                            const uint32_t* d_col, int nclouds, int published_lo, int published_hi, const char* call) {
  PLVS_HIP_TRY(h->updated.reserve((size_t)h->num_blocks + 1));
  bool second = false;
  PLVS_HIP_TRY(radix_sort_pairs(h->keys0.p, h->seq0.p, h->keys1.p, h->seq1.p, V, 0, voxel_key_bits(h->num_blocks), h->scratch.p, s,
                                &second));
  const uint32_t* keys = second ? h->keys1.p : h->keys0.p;
  const uint32_t* seqs = second ? h->seq1.p : h->seq0.p;
  // (Folding the records in slices on a second stream while the next slice is expanded was measured in round 3: the two
  // kernels slow each other down by more than the overlap gains — 1.03-1.13 ms with two slices, 1.08-1.20 with four,
  // against 0.93-1.03 for one after the other.)
  vb_launch_expand(h, s, mode, keys, seqs, V, d_xyz, d_aux, d_col, nclouds);
  PLVS_KERNEL_CHECK();
  hipLaunchKernelGGL(vb_chain_chunks, dim3(ceil_div(V, kChainChunk)), dim3(kChainThreads), 0, s, h->P, keys, V, h->rec.p,
                     h->rec_c.p, h->d_ctr, h->dist, h->weight, h->rgba);
  PLVS_KERNEL_CHECK();
  int rc = vb_read_counters(h, s);
  if (rc != PLVS_OK) return rc;
  if (h->h_ctr->err) {
    h->poisoned = true;
    plvs::set_error("tsdf_voxblox %s: internal directory miss (err=%u)", call, h->h_ctr->err);
    return PLVS_ERR_CAPACITY;
  }
  h->stats.updated_chunks = (int32_t)h->h_ctr->num_updated;
  h->stats.voxels = (int32_t)h->h_ctr->num_heads;
  h->stats.max_run = (int32_t)h->h_ctr->max_run;
  h->last_updated = h->h_ctr->num_updated;
  return vb_publish_waiting(h, s, published_lo, published_hi);
}

// One call of the ordered pipeline.  mode kSimple / kFast: camera clouds, the rays of a fast call cut by vb_fast_plan
// (fast_offset: the sets' offset of the first cloud).  mode kWorld: the world-cloud-with-normals flavour
// (integrateWorlPointCloud), d_aux = normals; mode kMerged:
// MergedTsdfIntegrator's bundles, d_aux = merged weights, d_clr = clearing flags.  Both: one cloud.
static int vb_integrate_impl(plvs_tsdf_voxblox* h, const float* d_xyz, const uint8_t* d_rgba, const int32_t* offsets, int nclouds,
                             const float* d_Twc, void* stream, int mode, const float* d_aux, const uint8_t* d_clr,
                             uint32_t fast_offset) {
  PLVS_REQUIRE(h, "null handle");
  PLVS_REQUIRE(!h->poisoned, "handle is in a failed state (clear it)");
  PLVS_REQUIRE(offsets && nclouds >= 0, "bad offsets");
  hipStream_t s = static_cast<hipStream_t>(stream);
  h->stats = plvs_tsdf_stats{};
  h->last_updated = 0;
  int n = 0;
  int rc = check_offsets(offsets, nclouds, &n);
  if (rc != PLVS_OK) return rc;
  h->stats.points = n;
  if (n == 0) return mode == kWorld ? PLVS_OK : vb_publish_all(h, s);   // (a world cloud publishes nothing: below)
  PLVS_REQUIRE(d_xyz && d_rgba && d_Twc, "null device pointer");
  PLVS_REQUIRE((reinterpret_cast<uintptr_t>(d_rgba) & 3) == 0, "rgba must be 4-byte aligned");
  rc = vb_halo_drop(h, s);   // new blocks go into the pool slots a meshing halo may still occupy
  if (rc != PLVS_OK) return rc;
  rc = vb_call_head(h, offsets, nclouds, d_Twc, s);
  if (rc != PLVS_OK) return rc;
  if (mode == kFast) {   // which rays are cast, and how far: the update counts take aux's place
    rc = vb_fast_plan(h, d_xyz, n, nclouds, h->poses.p, fast_offset, s);
    if (rc != PLVS_OK) return rc;
    d_aux = reinterpret_cast<const float*>(h->ff_L.p);
  }
  PLVS_HIP_TRY(h->counts.reserve((size_t)n));
  PLVS_HIP_TRY(h->scratch.reserve(scan_scratch_words((size_t)n)));
  vb_launch_ray_pass<false>(h, s, mode, d_xyz, d_aux, d_clr, n, nclouds);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(exclusive_scan_u32(h->counts.p, h->counts.p, (size_t)n, &h->d_ctr->total_visits, h->scratch.p, s));
  rc = vb_read_counters(h, s);
  if (rc != PLVS_OK) return rc;
  if (h->h_ctr->err) return vb_fail(h, "integrate", h->h_ctr->err);
  const uint32_t V = h->h_ctr->total_visits;
  const int before = h->num_blocks;
  h->num_blocks = h->h_ctr->num_blocks;
  // integratePointCloud starts with updateLayerWithStoredBlocks (tsdf_integrator.cc:306, :343): whatever a world cloud
  // left waiting joins the layer now; integrateWorlPointCloud itself never calls it (:35-82)
  const int published_lo = h->visible_blocks, published_hi = (mode == kWorld && h->defer_world_blocks) ? h->visible_blocks : before;
  if (!(mode == kWorld && h->defer_world_blocks)) h->visible_blocks = h->num_blocks;
  h->stats.visits = V;
  h->stats.new_chunks = h->num_blocks - before;
  if (V == 0) return vb_publish_waiting(h, s, published_lo, published_hi);
  rc = vb_reserve_visits(h, V);
  if (rc != PLVS_OK) return rc;
  vb_launch_ray_pass<true>(h, s, mode, d_xyz, d_aux, d_clr, n, nclouds);
  PLVS_KERNEL_CHECK();
  rc = vb_sort_and_fold(h, s, mode, V, d_xyz, d_aux, reinterpret_cast<const uint32_t*>(d_rgba), nclouds, published_lo, published_hi,
                        "integrate");
  if (rc != PLVS_OK) return rc;
  if (h->visible_blocks < h->num_blocks && h->last_updated > 0) {   // Block::updated() of a block outside the layer is not seen
    hipLaunchKernelGGL(vb_filter_slots, dim3(1), dim3(1024), 0, s, h->updated.p, h->last_updated, (uint32_t)h->visible_blocks,
                       &h->d_ctr->num_updated);
    PLVS_KERNEL_CHECK();
    rc = vb_read_counters(h, s);
    if (rc != PLVS_OK) return rc;
    h->last_updated = h->h_ctr->num_updated;
  }
  return PLVS_OK;
}

// A host cloud (and its normals, if it has any) and its pose into the handle's staging buffers.
static int vb_stage_cloud(plvs_tsdf_voxblox* h, const float* xyz, const uint8_t* rgba, const float* normals, int n, const float* Twc) {
  PLVS_HIP_TRY(h->st_xyz.reserve((size_t)n * 3));
  PLVS_HIP_TRY(h->st_rgba.reserve((size_t)n));
  PLVS_HIP_TRY(h->st_Twc.reserve(12));
  if (normals) PLVS_HIP_TRY(h->st_nrm.reserve((size_t)n * 3));
  PLVS_HIP_TRY(hipMemcpy(h->st_xyz.p, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->st_rgba.p, rgba, (size_t)n * 4, hipMemcpyHostToDevice));
  if (normals) PLVS_HIP_TRY(hipMemcpy(h->st_nrm.p, normals, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->st_Twc.p, Twc, 12 * sizeof(float), hipMemcpyHostToDevice));
  return PLVS_OK;
}

// A scan without points: it still publishes what a world cloud left waiting; a fast one still moves the sets on.
static int vb_empty_scan(plvs_tsdf_voxblox* h, bool fast = false) {
  const int32_t none[2] = {0, 0};
  return fast ? plvs_hip_tsdf_voxblox_integrate_fast_batch_dev(h, nullptr, nullptr, none, 1, nullptr, nullptr)
              : plvs_hip_tsdf_voxblox_integrate_batch_dev(h, nullptr, nullptr, none, 1, nullptr, nullptr);
}
