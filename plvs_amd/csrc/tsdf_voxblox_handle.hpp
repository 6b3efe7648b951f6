// The map handle of the voxblox back end and what every pipeline that works on it shares: the per-call counters, the kernel
// that publishes them and their read, the flush of the queue in front of every entry point, the meshers' view of the map, the
// failure path.  tsdf_voxblox.hip and the tsdf_voxblox_*.hpp headers of its pipelines (one translation unit) include it.
#pragma once
#include <vector>

#include "common.hpp"
#include "device_utils.hpp"
#include "tsdf_directory.hpp"
#include "tsdf_voxblox_core.hpp"
#include "tsdf_voxblox_view.hpp"

using namespace plvs;   // (a private header of one translation unit)
using namespace plvs::tsdf;
using namespace plvs::vbx;

namespace {

constexpr uint32_t kErrNonFinite = 8u;   // (beside the directory's bits, tsdf_directory.hpp)

struct VCounters {
  uint32_t total_visits;
  int32_t num_blocks;
  uint32_t err;
  uint32_t num_heads;
  uint32_t num_updated;
  uint32_t max_run;
};

__global__ void vb_publish_counters(const VCounters* __restrict__ ctr, VCounters* __restrict__ host_ctr) {
  const uint32_t* a = reinterpret_cast<const uint32_t*>(ctr);
  uint32_t* b = reinterpret_cast<uint32_t*>(host_ctr);
  for (int k = threadIdx.x; k < (int)(sizeof(VCounters) / sizeof(uint32_t)); k += blockDim.x) b[k] = a[k];
  __threadfence_system();
}

}  // namespace

struct plvs_tsdf_voxblox {
  plvs_tsdf_voxblox_params prm;
  Params P;
  Directory dir;
  float* dist = nullptr;
  float* weight = nullptr;
  uint32_t* rgba = nullptr;
  VCounters* d_ctr = nullptr;
  VCounters* h_ctr = nullptr;
  int num_blocks = 0;
  int visible_blocks = 0;              // blocks the layer shows: all, unless world-cloud blocks wait for the next camera-ray call
  bool defer_world_blocks = false;
  bool poisoned = false;
  DevBuf<uint32_t> counts, keys0, keys1, seq0, seq1, heads, updated, scratch, rec_c;
  DevBuf<float2> rec;
  DevBuf<uint32_t> upd_merge;          // (the updated list when waiting world-cloud blocks join it)
  DevBuf<int32_t> offsets;
  DevBuf<float> st_xyz, st_Twc, st_nrm;
  DevBuf<uint32_t> st_rgba;
  DevBuf<PoseRt> poses;
  // merged integrator: per-point kinds / end voxels, the bundles (CSR) and their merged points
  DevBuf<uint8_t> mg_kind, mg_clr;
  DevBuf<int32_t> mg_g;
  DevBuf<uint32_t> mg_first, mg_pts, mg_col;
  DevBuf<float> mg_xyz, mg_w;
  // fast integrator (tsdf_voxblox_fast.hpp): the two approximate sets as the reference keeps them, the offset of the next
  // scan, and the scratch of the rounds
  DevBuf<unsigned long long> ap_start, ap_seen, ff_shash, ff_qhash;
  DevBuf<uint32_t> ff_skey0, ff_skey1, ff_sval0, ff_sval1, ff_full, ff_Q, ff_L, ff_qoff, ff_qkey0, ff_qkey1, ff_qval0, ff_qval1, ff_flags;
  DevBuf<uint8_t> ff_seen;
  uint32_t* h_ff = nullptr;            // pinned: {queries of the next round, did a ray change}
  uint32_t ap_next = 1;                // (the reference's sets start at offset 0 and every scan begins with offset + 1)
  bool ap_ready = false;
  int fast_rounds = 0;                 // rounds of the last fast call (diagnostic)
  bool fast_sequential = false;        //   ... and whether it was finished on one thread (vbf_sequential)
  // queued key-frame clouds (plvs_hip_tsdf_voxblox_queue / _flush): uploaded, not yet integrated
  DevBuf<float> q_xyz, q_Twc_dev;   // (the poses get a buffer of their own: a host-flavour integrate that finds a queue has
                                    //  staged ITS pose in st_Twc already)
  DevBuf<uint32_t> q_rgba;
  std::vector<int32_t> q_offsets;   // [clouds + 1] once anything is queued
  std::vector<float> q_Twc;         // 12 per cloud
  plvs_tsdf_stats stats{};
  uint32_t last_updated = 0;
  void* ext = nullptr;                 // meshing scratch (tsdf_voxblox_mesh.hip), freed with the map
  void (*ext_free)(void*) = nullptr;
  // halo of a sharded map (meshing): ghost copies of other ranks' blocks in the pool slots past num_blocks
  Directory gdir{};
  int ghost_count = 0;
  DevBuf<uint32_t> halo_row;
  // ray-sharded integrate (tsdf_voxblox_shard.hpp): this rank's visit records in sequence order, their destinations and the
  // stable partition by destination; the owner's translated keys
  DevBuf<uint4> sv_rec;
  DevBuf<uint32_t> sv_dest, sv_dest1, sv_idx, sv_idx1, sv_cnt, sv_vkey, sv_seq;
  uint32_t* h_sv_cnt = nullptr;        // pinned: records per destination
  uint32_t sv_V = 0;
  int sv_phase = 0;                    // 0 idle, 1 walked, 2 packed
  bool sv_partitioned = false;
};

// Every entry point that reads or changes the map integrates the queued key-frame clouds first (plvs_hip_tsdf_voxblox_queue).
extern "C" int plvs_hip_tsdf_voxblox_flush(plvs_tsdf_voxblox* h);
#define VB_FLUSH_QUEUE(h)                                          \
  do {                                                             \
    if ((h) && !(h)->q_offsets.empty()) {                          \
      const int rc_flush_ = plvs_hip_tsdf_voxblox_flush(h);        \
      if (rc_flush_ != PLVS_OK) return rc_flush_;                  \
    }                                                              \
  } while (0)

namespace plvs {
namespace vbx {

bool voxblox_map_view(plvs_tsdf_voxblox* h, VoxbloxMapView* v) {
  if (h == nullptr || v == nullptr || h->poisoned) return false;
  if (!h->q_offsets.empty() && plvs_hip_tsdf_voxblox_flush(h) != PLVS_OK) return false;   // (the meshers read the map)
  v->voxel_size = h->P.voxel_size;
  v->voxel_size_inv = h->P.voxel_size_inv;
  v->dir = h->dir;
  v->distance = h->dist;
  v->weight = h->weight;
  v->rgba = h->rgba;
  v->num_blocks = h->num_blocks;
  v->visible_blocks = h->visible_blocks;
  v->shard_count = h->P.shard_count;
  v->ghost = h->gdir;
  v->ext = &h->ext;
  v->ext_free = &h->ext_free;
  return true;
}

}  // namespace vbx
}  // namespace plvs

static int vb_read_counters(plvs_tsdf_voxblox* h, hipStream_t s) {
  // (published by a kernel's stores into the pinned copy: a small copy command costs tens of microseconds of queueing)
  hipLaunchKernelGGL(vb_publish_counters, dim3(1), dim3(64), 0, s, h->d_ctr, h->h_ctr);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(hipStreamSynchronize(s));
  return PLVS_OK;
}

// ---- failure: the error word of a call's counters -> the text behind plvs_hip_last_error and the return code.  A call that
// may have changed the map poisons the handle (clear() revives it); shard_walk only reads the clouds (poison = false).
// A stage raises only the bits its kernels can set (the count pass no directory miss, shard_walk no full pool, shard_apply
// no non-finite point): the other texts stay empty for it.
static int vb_fail(plvs_tsdf_voxblox* h, const char* call, uint32_t err, bool poison = true) {
  if (poison) h->poisoned = true;
  plvs::set_error("tsdf_voxblox %s: %s%s%s%s", call, (err & kErrPoolFull) ? "block pool full (raise max_blocks) " : "",
                  (err & kErrCoordRange) ? "block id outside [-2^19, 2^19) " : "",
                  (err & kErrNonFinite) ? "non-finite point in the cloud " : "",
                  (err & kErrDirectoryMiss) ? "a record for a block of another rank " : "");
  return (err & kErrNonFinite) ? PLVS_ERR_INVALID_ARG : PLVS_ERR_CAPACITY;
}
