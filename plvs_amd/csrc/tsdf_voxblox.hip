// TSDF map of the voxblox back end (PointCloudMapVoxblox::InsertCloud -> TsdfServer::insertPointCloud ->
// SimpleTsdfIntegrator::integratePointCloud; the merged and fast integrators and the LoadMap path beside it): the C ABI
// of the map handle.
//
// Same device pipeline as the chisel path (tsdf_chisel_ordered.hpp): count -> scan ->
// fill -> stable radix sort by voxel -> expand (order-independent operands) ->
// chain (one thread folds each voxel's records in the reference's visiting
// order).  The visiting order is voxblox's ThreadSafeIndex "mixed" order; a
// record's sequence number is the position of its point in that order, so the
// single-thread schedule of the reference is reproduced exactly.
//
// HBM layout: three planes distance / weight / rgba of max_blocks*4096 dwords
// (12 B per voxel, 48 KiB per block, voxel.h:12-18), the shared block directory
// (tsdf_directory.hpp), and per call one (u32 key, u32 sequence) pair plus
// 12 B of operands per voxel visit.
//
// This file keeps the handle's life cycle, the entry points (argument checks, then a call into a header), the queue, the
// accessors and upload / download of a block; each concern has a header of its own, all one translation unit:
//   tsdf_voxblox_handle.hpp     the handle, its counters and their read, the queue flush, the failure path
//   tsdf_voxblox_kernels.hpp    kernels of the ordered pipeline (ray passes, expansion, fold)
//   tsdf_voxblox_integrate.hpp  its host side: head, count + scan, fill, tail; staging of host clouds
//   tsdf_voxblox_fast.hpp       FastTsdfIntegrator: which rays are cast and how far
//   tsdf_voxblox_merged.hpp     MergedTsdfIntegrator: the bundles and their order
//   tsdf_voxblox_shard.hpp      ray-sharded multi-GPU integrate
//   tsdf_voxblox_halo.hpp       halo of a sharded map (meshing)
#include <cstring>
#include <vector>

#include "tsdf_voxblox_handle.hpp"
#include "tsdf_voxblox_kernels.hpp"
#include "tsdf_voxblox_halo.hpp"
#include "tsdf_voxblox_integrate.hpp"
#include "tsdf_voxblox_fast.hpp"
#include "tsdf_voxblox_merged.hpp"
#include "tsdf_voxblox_shard.hpp"

extern "C" {

int plvs_hip_tsdf_voxblox_default_params(float voxel_size, int use_carving,
                                         plvs_tsdf_voxblox_params* p) {
  PLVS_REQUIRE(p, "params is null");
  PLVS_REQUIRE(voxel_size > 0.0f, "voxel_size must be positive");
  p->voxel_size = voxel_size;        // tsdf_voxel_size = PointCloudMapping.resolution
  p->truncation = 0.1f;              // src/PointCloudMapVoxblox.cc:57
  p->max_weight = 10000.0f;          // :58
  p->min_ray_length = 0.1f;          // :60
  p->max_ray_length = 5.0f;          // :61
  p->voxel_carving = use_carving ? 1 : 0;  // :59
  p->max_blocks = 32768;             // 1.5 GiB of voxel pool
  p->shard_rank = 0;
  p->shard_count = 1;
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_destroy(plvs_tsdf_voxblox* h) {
  if (!h) return PLVS_OK;
  if (h->ext && h->ext_free) h->ext_free(h->ext);
  (void)hipFree(h->gdir.keys); (void)hipFree(h->gdir.slots);
  h->halo_row.release();
  (void)hipFree(h->dir.keys); (void)hipFree(h->dir.slots); (void)hipFree(h->dir.slot_ids);
  (void)hipFree(h->dist); (void)hipFree(h->weight); (void)hipFree(h->rgba); (void)hipFree(h->d_ctr);
  if (h->h_ctr) (void)hipHostFree(h->h_ctr);
  if (h->h_ff) (void)hipHostFree(h->h_ff);
  if (h->h_sv_cnt) (void)hipHostFree(h->h_sv_cnt);
  h->sv_rec.release(); h->sv_dest.release(); h->sv_dest1.release(); h->sv_idx.release(); h->sv_idx1.release(); h->sv_cnt.release();
  h->sv_vkey.release(); h->sv_seq.release();
  h->q_xyz.release(); h->q_rgba.release(); h->q_Twc_dev.release();
  h->ap_start.release(); h->ap_seen.release(); h->ff_shash.release(); h->ff_qhash.release(); h->ff_skey0.release(); h->ff_skey1.release();
  h->ff_sval0.release(); h->ff_sval1.release(); h->ff_full.release(); h->ff_Q.release(); h->ff_L.release(); h->ff_qoff.release();
  h->ff_qkey0.release(); h->ff_qkey1.release(); h->ff_qval0.release(); h->ff_qval1.release(); h->ff_flags.release(); h->ff_seen.release();
  h->counts.release(); h->keys0.release(); h->keys1.release(); h->seq0.release(); h->seq1.release();
  h->heads.release(); h->updated.release(); h->scratch.release(); h->rec_c.release(); h->rec.release(); h->upd_merge.release();
  h->offsets.release(); h->st_xyz.release(); h->st_Twc.release(); h->st_nrm.release(); h->st_rgba.release();
  h->mg_kind.release(); h->mg_clr.release(); h->mg_g.release(); h->mg_first.release(); h->mg_pts.release(); h->mg_col.release();
  h->mg_xyz.release(); h->mg_w.release(); h->poses.release();
  delete h;
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_clear(plvs_tsdf_voxblox* h) {
  PLVS_REQUIRE(h, "null handle");
  if (h->gdir.keys != nullptr) PLVS_HIP_TRY(hipMemset(h->gdir.keys, 0xFF, ((size_t)h->gdir.mask + 1) * sizeof(unsigned long long)));
  h->ghost_count = 0;
  const size_t cap = (size_t)h->dir.mask + 1;
  const size_t nvox = (size_t)h->prm.max_blocks * kBlockVox;
  PLVS_HIP_TRY(hipMemset(h->dir.keys, 0xFF, cap * sizeof(unsigned long long)));
  PLVS_HIP_TRY(hipMemset(h->dir.slots, 0xFF, cap * sizeof(int32_t)));
  PLVS_HIP_TRY(hipMemset(h->dist, 0, nvox * sizeof(float)));     // TsdfVoxel defaults: 0, 0, Color()
  PLVS_HIP_TRY(hipMemset(h->weight, 0, nvox * sizeof(float)));
  PLVS_HIP_TRY(hipMemset(h->rgba, 0, nvox * sizeof(uint32_t)));
  PLVS_HIP_TRY(hipMemset(h->d_ctr, 0, sizeof(VCounters)));
  PLVS_HIP_TRY(hipDeviceSynchronize());
  h->num_blocks = 0;
  h->visible_blocks = 0;
  h->poisoned = false;
  h->stats = plvs_tsdf_stats{};
  h->last_updated = 0;
  h->ap_ready = false;   // (a new map = a new integrator: fresh sets, offset 0)
  h->ap_next = 1;
  h->q_offsets.clear();  // (queued clouds belong to the map that is gone)
  h->q_Twc.clear();
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_create(const plvs_tsdf_voxblox_params* p, plvs_tsdf_voxblox** out) {
  PLVS_REQUIRE(p && out, "null argument");
  PLVS_REQUIRE(p->voxel_size > 0.0f, "voxel_size must be positive");
  PLVS_REQUIRE(p->max_blocks > 0 && p->max_blocks <= (1 << 20), "max_blocks must be in (0, 2^20]");
  PLVS_REQUIRE(p->shard_count <= 1 || (p->shard_rank >= 0 && p->shard_rank < p->shard_count),
               "shard_rank out of range");
  plvs_tsdf_voxblox* h = new plvs_tsdf_voxblox();
  h->prm = *p;
  Params& P = h->P;
  P.voxel_size = p->voxel_size;
  P.voxel_size_inv = (float)(1.0 / p->voxel_size);  // tsdf_integrator.cc:17
  P.vps_inv = (float)(1.0 / 16);                    // :19
  P.truncation = p->truncation;
  P.max_weight = p->max_weight;
  P.min_ray = p->min_ray_length;
  P.max_ray = p->max_ray_length;
  P.carving = p->voxel_carving ? 1 : 0;
  P.allow_clear = P.carving;  // allow_clear = true in PLVS, but it needs carving (:26-28)
  P.shard_rank = p->shard_rank;
  P.shard_count = p->shard_count < 1 ? 1 : p->shard_count;
  uint32_t cap = 1024;
  while (cap < 2u * (uint32_t)p->max_blocks) cap <<= 1;
  h->dir.mask = cap - 1;
  h->dir.max_blocks = p->max_blocks;
  const size_t nvox = (size_t)p->max_blocks * kBlockVox;
#define VB_TRY(call)                                                            \
  do {                                                                          \
    hipError_t _e = (call);                                                     \
    if (_e != hipSuccess) {                                                     \
      plvs::set_error("%s failed: %s", #call, hipGetErrorString(_e));          \
      plvs_hip_tsdf_voxblox_destroy(h);                                         \
      return PLVS_ERR_HIP;                                                      \
    }                                                                           \
  } while (0)
  VB_TRY(hipMalloc((void**)&h->dir.keys, (size_t)cap * sizeof(unsigned long long)));
  VB_TRY(hipMalloc((void**)&h->dir.slots, (size_t)cap * sizeof(int32_t)));
  VB_TRY(hipMalloc((void**)&h->dir.slot_ids, (size_t)p->max_blocks * 3 * sizeof(int32_t)));
  VB_TRY(hipMalloc((void**)&h->dist, nvox * sizeof(float)));
  VB_TRY(hipMalloc((void**)&h->weight, nvox * sizeof(float)));
  VB_TRY(hipMalloc((void**)&h->rgba, nvox * sizeof(uint32_t)));
  VB_TRY(hipMalloc((void**)&h->d_ctr, sizeof(VCounters)));
  VB_TRY(hipHostMalloc((void**)&h->h_ctr, sizeof(VCounters)));
#undef VB_TRY
  *out = h;
  int rc = plvs_hip_tsdf_voxblox_clear(h);
  if (rc != PLVS_OK) {
    plvs_hip_tsdf_voxblox_destroy(h);
    *out = nullptr;
  }
  return rc;
}

// Creates or REPLACES one block with the given voxel planes (host, 4096 each, index x + 16 * (y + 16 * z)): what
// Layer::addBlockFromProto does with BlockMergingStrategy::kReplace for every block of a saved layer
// (TsdfServer::loadMap, tsdf_server.cc:865-872 -> io::LoadBlocksFromFile; core/layer_inl.h:195-197, :215) once the
// protobuf has been read on the host.  The caller marks the block updated, as layer_inl.h:215 does.
int plvs_hip_tsdf_voxblox_upload_block(plvs_tsdf_voxblox* h, int bx, int by, int bz, const float* distance, const float* weight,
                                       const uint32_t* rgba) {
  PLVS_REQUIRE(h && distance && weight && rgba, "null argument");
  VB_FLUSH_QUEUE(h);
  PLVS_REQUIRE(!h->poisoned, "handle is in a failed state (clear it)");
  if (h->P.shard_count > 1)
    PLVS_REQUIRE(shard_of(owner_hash(bx, by, bz), h->P.shard_count) == h->P.shard_rank, "the block belongs to another rank");
  int rc = vb_halo_drop(h, nullptr);
  if (rc != PLVS_OK) return rc;
  PLVS_HIP_TRY(hipMemset(&h->d_ctr->err, 0, sizeof(uint32_t)));
  int32_t* d_slot = reinterpret_cast<int32_t*>(&h->d_ctr->total_visits);   // (a counter no call is using now)
  hipLaunchKernelGGL(vb_block_slot_of, dim3(1), dim3(64), 0, nullptr, h->dir, bx, by, bz, h->d_ctr, d_slot);
  PLVS_KERNEL_CHECK();
  rc = vb_read_counters(h, nullptr);
  if (rc != PLVS_OK) return rc;
  if (h->h_ctr->err) {
    h->poisoned = true;
    plvs::set_error("upload_block: %s", (h->h_ctr->err & kErrPoolFull) ? "block pool full (raise max_blocks)" : "block id outside [-2^19, 2^19)");
    return PLVS_ERR_CAPACITY;
  }
  const int slot = (int)h->h_ctr->total_visits;
  PLVS_REQUIRE(slot >= 0, "internal: the block was not inserted");
  h->num_blocks = h->h_ctr->num_blocks;
  h->visible_blocks = h->num_blocks;   // (a block handed to the layer directly: whatever waited joins with it)
  const size_t off = (size_t)slot * kBlockVox;
  PLVS_HIP_TRY(hipMemcpy(h->dist + off, distance, kBlockVox * sizeof(float), hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->weight + off, weight, kBlockVox * sizeof(float), hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->rgba + off, rgba, kBlockVox * sizeof(uint32_t), hipMemcpyHostToDevice));
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_halo_lookup(plvs_tsdf_voxblox* h, const int32_t* d_ids_xyz, int n, uint32_t* d_found, void* stream) {
  PLVS_REQUIRE(h && !h->poisoned, "unusable handle");
  VB_FLUSH_QUEUE(h);
  PLVS_REQUIRE(n >= 0, "negative size");
  if (n == 0) return PLVS_OK;
  PLVS_REQUIRE(d_ids_xyz && d_found, "null argument");
  return halo_lookup(h, d_ids_xyz, n, d_found, static_cast<hipStream_t>(stream));
}

int plvs_hip_tsdf_voxblox_halo_export(plvs_tsdf_voxblox* h, const int32_t* d_ids_xyz, const uint32_t* d_found, int n,
                                      uint32_t* d_payload, void* stream) {
  PLVS_REQUIRE(h && !h->poisoned, "unusable handle");
  VB_FLUSH_QUEUE(h);
  PLVS_REQUIRE(n >= 0, "negative size");
  if (n == 0 || d_payload == nullptr) return PLVS_OK;   // (no payload buffer: the caller saw no flag set)
  PLVS_REQUIRE(d_ids_xyz && d_found, "null argument");
  return halo_export(h, d_ids_xyz, d_found, n, d_payload, static_cast<hipStream_t>(stream));
}

int plvs_hip_tsdf_voxblox_halo_import(plvs_tsdf_voxblox* h, const int32_t* d_ids_xyz, const uint32_t* d_found,
                                      const uint32_t* d_payload, int n, int nfound, void* stream) {
  PLVS_REQUIRE(h && !h->poisoned, "unusable handle");
  VB_FLUSH_QUEUE(h);
  PLVS_REQUIRE(n >= 0 && nfound >= 0 && nfound <= n, "bad sizes");
  if (n == 0 || nfound == 0) return PLVS_OK;
  PLVS_REQUIRE(d_ids_xyz && d_found && d_payload, "null argument");
  return halo_import(h, d_ids_xyz, d_found, d_payload, n, nfound, static_cast<hipStream_t>(stream));
}

int plvs_hip_tsdf_voxblox_halo_clear(plvs_tsdf_voxblox* h) {
  PLVS_REQUIRE(h, "null handle");
  VB_FLUSH_QUEUE(h);
  return halo_clear(h);
}

int plvs_hip_tsdf_voxblox_integrate_batch_dev(plvs_tsdf_voxblox* h, const float* d_xyz,
                                              const uint8_t* d_rgba, const int32_t* offsets,
                                              int nclouds, const float* d_Twc, void* stream) {
  VB_FLUSH_QUEUE(h);
  return vb_integrate_impl(h, d_xyz, d_rgba, offsets, nclouds, d_Twc, stream, kSimple, nullptr, nullptr, 0);
}

// ---- the ray-sharded integrate (tsdf_voxblox_shard.hpp)
int plvs_hip_tsdf_voxblox_shard_walk(plvs_tsdf_voxblox* h, const float* d_xyz, const int32_t* offsets, int nclouds,
                                     const float* d_Twc, int64_t* send_counts, void* stream) {
  PLVS_REQUIRE(h && offsets && send_counts && nclouds >= 0, "bad argument");
  PLVS_REQUIRE(!h->poisoned, "handle is in a failed state (clear it)");
  VB_FLUSH_QUEUE(h);
  return vb_shard_walk(h, d_xyz, offsets, nclouds, d_Twc, send_counts, static_cast<hipStream_t>(stream));
}

int plvs_hip_tsdf_voxblox_shard_pack(plvs_tsdf_voxblox* h, void* d_send, void* stream) {
  PLVS_REQUIRE(h, "null handle");
  PLVS_REQUIRE(h->sv_phase == 1, "shard_pack follows shard_walk");
  return vb_shard_pack(h, d_send, static_cast<hipStream_t>(stream));
}

int plvs_hip_tsdf_voxblox_shard_apply(plvs_tsdf_voxblox* h, const void* d_recv, const int64_t* recv_counts, const float* d_xyz,
                                      const uint8_t* d_rgba, const int32_t* offsets, int nclouds, const float* d_Twc, void* stream) {
  PLVS_REQUIRE(h && recv_counts && offsets && nclouds >= 0, "bad argument");
  PLVS_REQUIRE(!h->poisoned, "handle is in a failed state (clear it)");
  PLVS_REQUIRE(h->sv_phase == 2, "shard_apply follows shard_pack");
  return vb_shard_apply(h, d_recv, recv_counts, d_xyz, d_rgba, offsets, nclouds, d_Twc, static_cast<hipStream_t>(stream));
}

int plvs_hip_tsdf_voxblox_integrate_fast_batch_dev(plvs_tsdf_voxblox* h, const float* d_xyz, const uint8_t* d_rgba,
                                                   const int32_t* offsets, int nclouds, const float* d_Twc, void* stream) {
  PLVS_REQUIRE(h, "null handle");
  VB_FLUSH_QUEUE(h);
  PLVS_REQUIRE(offsets && nclouds >= 0, "bad offsets");
  return vb_integrate_fast_batches(h, d_xyz, d_rgba, offsets, nclouds, d_Twc, stream);
}

int plvs_hip_tsdf_voxblox_integrate_fast(plvs_tsdf_voxblox* h, const float* xyz, const uint8_t* rgba, int n, const float* Twc) {
  PLVS_REQUIRE(h, "null handle");
  VB_FLUSH_QUEUE(h);
  PLVS_REQUIRE(n >= 0 && Twc, "bad arguments");
  if (n == 0) return vb_empty_scan(h, true);   // (an empty scan still moves the sets on)
  PLVS_REQUIRE(xyz && rgba, "null cloud pointer");
  int rc = vb_stage_cloud(h, xyz, rgba, nullptr, n, Twc);
  if (rc != PLVS_OK) return rc;
  const int32_t offsets[2] = {0, n};
  rc = plvs_hip_tsdf_voxblox_integrate_fast_batch_dev(h, h->st_xyz.p, reinterpret_cast<const uint8_t*>(h->st_rgba.p), offsets, 1,
                                                      h->st_Twc.p, nullptr);
  if (rc != PLVS_OK) return rc;
  PLVS_HIP_TRY(hipDeviceSynchronize());
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_fast_rounds(plvs_tsdf_voxblox* h, int* rounds) {
  PLVS_REQUIRE(h && rounds, "null argument");
  *rounds = h->fast_rounds;
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_integrate_world_normals(plvs_tsdf_voxblox* h, const float* xyz, const uint8_t* rgba,
                                                  const float* normals, int n, const float* Twc) {
  PLVS_REQUIRE(h, "null handle");
  VB_FLUSH_QUEUE(h);
  PLVS_REQUIRE(n >= 0 && Twc, "bad arguments");
  if (n == 0) {
    h->stats = plvs_tsdf_stats{};
    h->last_updated = 0;
    return PLVS_OK;
  }
  PLVS_REQUIRE(xyz && rgba && normals, "null cloud pointer");
  int rc = vb_stage_cloud(h, xyz, rgba, normals, n, Twc);
  if (rc != PLVS_OK) return rc;
  const int32_t offsets[2] = {0, n};
  rc = vb_integrate_impl(h, h->st_xyz.p, reinterpret_cast<const uint8_t*>(h->st_rgba.p), offsets, 1, h->st_Twc.p, nullptr, kWorld,
                         h->st_nrm.p, nullptr, 0);
  (void)hipDeviceSynchronize();
  return rc;
}

int plvs_hip_tsdf_voxblox_integrate_merged(plvs_tsdf_voxblox* h, const float* xyz, const uint8_t* rgba, int n,
                                           const float* Twc) {
  PLVS_REQUIRE(h, "null handle");
  VB_FLUSH_QUEUE(h);
  PLVS_REQUIRE(n >= 0 && Twc, "bad arguments");
  PLVS_REQUIRE(!h->poisoned, "handle is in a failed state (clear it)");
  return vb_integrate_merged(h, xyz, rgba, n, Twc);
}

// Queued insertion, as for the chisel map (plvs_hip_tsdf_chisel_queue): PLVS inserts one key frame per InsertCloud and reads
// the layer only in UpdateMap (src/PointCloudMapping.cc:537-556, 594-598; PointCloudMapVoxblox::UpdateMap :160-179).  _queue
// uploads and returns, _flush integrates what waits as ONE batch of the simple integrator — every cloud a scan of its own,
// in order: the layer of the call-by-call sequence, bit for bit.  Every entry point that reads or changes the map flushes
// first; clear drops the queue.
int plvs_hip_tsdf_voxblox_queue(plvs_tsdf_voxblox* h, const float* xyz, const uint8_t* rgba, int n, const float* Twc) {
  PLVS_REQUIRE(h, "null handle");
  PLVS_REQUIRE(n >= 0 && Twc, "bad arguments");
  PLVS_REQUIRE(n == 0 || (xyz && rgba), "null cloud pointer");
  const bool first = h->q_offsets.empty();
  const size_t at = first ? 0 : (size_t)h->q_offsets.back();
  PLVS_REQUIRE(at + (size_t)n < 0x7FFFFFFFull, "too many queued points");
  if (n) {
    PLVS_HIP_TRY(grow_keep(h->q_xyz, 3 * at, 3 * (at + (size_t)n)));
    PLVS_HIP_TRY(grow_keep(h->q_rgba, at, at + (size_t)n));
    PLVS_HIP_TRY(hipMemcpy(h->q_xyz.p + 3 * at, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
    PLVS_HIP_TRY(hipMemcpy(h->q_rgba.p + at, rgba, (size_t)n * 4, hipMemcpyHostToDevice));
  }
  if (first) h->q_offsets.push_back(0);
  h->q_offsets.push_back((int32_t)(at + (size_t)n));   // (an empty cloud is a scan too: it publishes waiting blocks)
  h->q_Twc.insert(h->q_Twc.end(), Twc, Twc + 12);
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_queued(plvs_tsdf_voxblox* h, int* nclouds) {
  PLVS_REQUIRE(h && nclouds, "null argument");
  *nclouds = h->q_offsets.empty() ? 0 : (int)h->q_offsets.size() - 1;
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_flush(plvs_tsdf_voxblox* h) {
  PLVS_REQUIRE(h, "null handle");
  if (h->q_offsets.empty()) return PLVS_OK;
  const int nclouds = (int)h->q_offsets.size() - 1;
  std::vector<int32_t> offsets;
  std::vector<float> Twc;
  offsets.swap(h->q_offsets);   // (the queue is empty from here on: the integrate below flushes nothing)
  Twc.swap(h->q_Twc);
  PLVS_HIP_TRY(h->q_Twc_dev.reserve((size_t)12 * nclouds));
  PLVS_HIP_TRY(hipMemcpy(h->q_Twc_dev.p, Twc.data(), (size_t)12 * nclouds * sizeof(float), hipMemcpyHostToDevice));
  int rc = plvs_hip_tsdf_voxblox_integrate_batch_dev(h, h->q_xyz.p, reinterpret_cast<const uint8_t*>(h->q_rgba.p), offsets.data(), nclouds,
                                                     h->q_Twc_dev.p, nullptr);
  if (rc != PLVS_OK) {
    // The queue was taken before the batch ran (a reader that flushes must not flush again from inside it): its clouds are
    // gone.  Say so, and how many — the error surfaces from whichever call triggered the flush, possibly a reader.
    char own[400];
    snprintf(own, sizeof own, "%s", plvs::last_error_buf());
    plvs::set_error("%s — raised by the flush of %d queued key-frame cloud%s (plvs_hip_tsdf_voxblox_queue): NONE of them was "
                    "integrated and they are dropped; queue them again after clearing / enlarging the map", own, nclouds,
                    nclouds == 1 ? "" : "s");
    return rc;
  }
  PLVS_HIP_TRY(hipDeviceSynchronize());
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_integrate(plvs_tsdf_voxblox* h, const float* xyz, const uint8_t* rgba,
                                    int n, const float* Twc) {
  PLVS_REQUIRE(h, "null handle");
  VB_FLUSH_QUEUE(h);
  PLVS_REQUIRE(n >= 0 && Twc, "bad arguments");
  if (n == 0) return vb_empty_scan(h);   // (an empty cloud still publishes what a world cloud left waiting)
  PLVS_REQUIRE(xyz && rgba, "null cloud pointer");
  int rc = vb_stage_cloud(h, xyz, rgba, nullptr, n, Twc);
  if (rc != PLVS_OK) return rc;
  const int32_t offsets[2] = {0, n};
  rc = plvs_hip_tsdf_voxblox_integrate_batch_dev(
      h, h->st_xyz.p, reinterpret_cast<const uint8_t*>(h->st_rgba.p), offsets, 1, h->st_Twc.p, nullptr);
  if (rc != PLVS_OK) return rc;
  PLVS_HIP_TRY(hipDeviceSynchronize());
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_set_deferred_world_blocks(plvs_tsdf_voxblox* h, int enable) {
  PLVS_REQUIRE(h, "null handle");
  VB_FLUSH_QUEUE(h);
  h->defer_world_blocks = enable != 0;
  if (!h->defer_world_blocks) h->visible_blocks = h->num_blocks;
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_last_stats(plvs_tsdf_voxblox* h, plvs_tsdf_stats* s) {
  PLVS_REQUIRE(h && s, "null argument");
  VB_FLUSH_QUEUE(h);
  *s = h->stats;
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_num_blocks(plvs_tsdf_voxblox* h, int* n) {
  PLVS_REQUIRE(h && n, "null argument");
  VB_FLUSH_QUEUE(h);
  *n = h->visible_blocks;
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_block_ids(plvs_tsdf_voxblox* h, int32_t* ids_xyz, int cap, int* n) {
  PLVS_REQUIRE(h && n, "null argument");
  VB_FLUSH_QUEUE(h);
  *n = h->visible_blocks;
  const int m = h->visible_blocks < cap ? h->visible_blocks : cap;
  if (m > 0) {
    PLVS_REQUIRE(ids_xyz, "null output");
    PLVS_HIP_TRY(hipMemcpy(ids_xyz, h->dir.slot_ids, (size_t)m * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_updated_block_ids_dev(plvs_tsdf_voxblox* h, int32_t* d_ids_xyz, int cap,
                                                int* n, void* stream) {
  PLVS_REQUIRE(h && n, "null argument");
  VB_FLUSH_QUEUE(h);
  *n = (int)h->last_updated;
  const int m = (int)h->last_updated < cap ? (int)h->last_updated : cap;
  if (m <= 0) return PLVS_OK;
  PLVS_REQUIRE(d_ids_xyz, "null output");
  hipLaunchKernelGGL(vb_gather_slot_ids, dim3(ceil_div((size_t)m, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), h->updated.p, m, h->dir.slot_ids, d_ids_xyz);
  PLVS_KERNEL_CHECK();
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_updated_block_ids(plvs_tsdf_voxblox* h, int32_t* ids_xyz, int cap, int* n) {
  PLVS_REQUIRE(h && n, "null argument");
  VB_FLUSH_QUEUE(h);
  *n = (int)h->last_updated;
  const int m = (int)h->last_updated < cap ? (int)h->last_updated : cap;
  if (m <= 0) return PLVS_OK;
  PLVS_REQUIRE(ids_xyz, "null output");
  // small lists: resolve slot -> id on the host
  std::vector<uint32_t> slots(h->last_updated);
  std::vector<int32_t> all((size_t)h->num_blocks * 3);
  PLVS_HIP_TRY(hipMemcpy(slots.data(), h->updated.p, slots.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  PLVS_HIP_TRY(hipMemcpy(all.data(), h->dir.slot_ids, all.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int i = 0; i < m; ++i) memcpy(ids_xyz + 3 * i, all.data() + 3 * (size_t)slots[(size_t)i], 3 * sizeof(int32_t));
  return PLVS_OK;
}

int plvs_hip_tsdf_voxblox_download_block(plvs_tsdf_voxblox* h, int bx, int by, int bz,
                                         float* distance, float* weight, uint32_t* rgba) {
  PLVS_REQUIRE(h && distance && weight && rgba, "null argument");
  VB_FLUSH_QUEUE(h);
  std::vector<int32_t> all((size_t)h->num_blocks * 3);
  if (h->num_blocks > 0)
    PLVS_HIP_TRY(hipMemcpy(all.data(), h->dir.slot_ids, all.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  int slot = -1;
  for (int i = 0; i < h->visible_blocks; ++i)
    if (all[3 * i] == bx && all[3 * i + 1] == by && all[3 * i + 2] == bz) { slot = i; break; }
  if (slot < 0) {
    plvs::set_error("block (%d,%d,%d) does not exist", bx, by, bz);
    return PLVS_ERR_INVALID_ARG;
  }
  const size_t off = (size_t)slot * kBlockVox;
  PLVS_HIP_TRY(hipMemcpy(distance, h->dist + off, kBlockVox * sizeof(float), hipMemcpyDeviceToHost));
  PLVS_HIP_TRY(hipMemcpy(weight, h->weight + off, kBlockVox * sizeof(float), hipMemcpyDeviceToHost));
  PLVS_HIP_TRY(hipMemcpy(rgba, h->rgba + off, kBlockVox * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return PLVS_OK;
}

}  // extern "C"

#if PLVS_VB_PROF
extern "C" int plvs_hip_debug_chain_prof(unsigned long long* out, int nwaves) {
  PLVS_HIP_TRY(hipDeviceSynchronize());
  PLVS_HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chain_prof), (size_t)nwaves * 4 * sizeof(unsigned long long)));
  return PLVS_OK;
}
#endif
