// Ray-sharded multi-GPU integrate of the voxblox back end (SimpleTsdfIntegrator; one of the headers of tsdf_voxblox.hip's translation unit).  New
// design: the reference is a single process.
//
// The map is sharded by block (owner = three-prime AnyIndexHash mod N, block_hash.h:21-24), the WORK by key frame: rank r
// casts the rays of the clouds c = r (mod N) of every call — through whatever blocks they cross — and every voxel
// visit travels to the block's owner as a 16-byte record {block id (packed, 8 B), voxel | cloud << 12, sequence number
// of the ray}.  updateTsdfVoxel is order dependent (clamp, float blend), so the owner applies a voxel's visits in the
// reference's order: the sequence numbers are GLOBAL (cloud after cloud, the mixed order inside a cloud), a sender's
// records leave in sequence order (a stable partition by destination), the owner sorts what it received by cloud and then
// by voxel (stable radix passes) and runs the single-device pipeline's expansion and fold on it — the operands of a
// visit are recomputed from (point, voxel) at the owner, which holds the same clouds.  The union of the shards is the
// single-device layer bit for bit, whatever N is (tests/test_tsdf_voxblox_shard.py).  Before (rounds 1-3) every rank cast
// every ray and kept the visits of its own blocks: the walk — a fifth of a call — did not scale.
//
//   shard_walk    count pass + fill pass over this rank's clouds (no directory: block ids come from the voxel grid),
//                 records in sequence order; destination of every record, stable partition -> send counts
//   shard_pack    the records grouped by destination, in the caller's send buffer
//   (exchange)    counts, then ONE all-to-all of the records
//   shard_apply   block id -> slot of the owner's directory (first-touch blocks inserted), sort by cloud, sort by voxel,
//                 vb_expand, vb_chain_chunks
#pragma once
#include <algorithm>

#include "tsdf_voxblox_integrate.hpp"

namespace {
namespace {   // (nested: the kernels keep the symbol names they had inside tsdf_voxblox.hip's own namespace)

constexpr uint32_t kVbWire = 4;   // 32-bit words of a visit record on the wire

template <bool kFill>
__global__ __launch_bounds__(256) void vb_shard_ray_pass(Params P, const float* __restrict__ xyz, int npoints,
                                                         const int32_t* __restrict__ offsets, int nclouds,
                                                         const PoseRt* __restrict__ Twc, int rank, int nranks,
                                                         VCounters* __restrict__ ctr, uint32_t* __restrict__ counts,
                                                         uint4* __restrict__ rec, uint32_t* __restrict__ dest) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;   // sequence position
  if (i >= npoints) return;
  uint32_t n = 0;
  const uint32_t out = kFill ? counts[i] : 0u;
  int cloud = 0;
  const int p = point_of_seq(offsets, nclouds, i, &cloud);
  if (cloud % nranks == rank) {
    const float px = xyz[3 * (size_t)p], py = xyz[3 * (size_t)p + 1], pz = xyz[3 * (size_t)p + 2];
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) {
      if (!kFill) atomicOr(&ctr->err, kErrNonFinite);
    } else {
      const PoseRt pose = load_pose(Twc, cloud);
      Ray ray;
      if (make_ray(P, pose, px, py, pz, &ray, false)) {
        const int steps = ray.steps < kMaxRaySteps ? ray.steps : kMaxRaySteps;
        for (int s = 0; s <= steps; ++s) {
          int g[3], b[3], vid;
          ray_step(&ray, g);
          if (!block_of(P, g, b, &vid)) continue;   // (P.shard_count = 1 here: never)
          unsigned long long key = 0;
          const bool in_range = pack_block(b[0], b[1], b[2], &key) && block_id_in_range(b[0], b[1], b[2]) &&
                                ((((g[0] - b[0] * 16) | (g[1] - b[1] * 16) | (g[2] - b[2] * 16)) & ~15) == 0);
          if (!kFill && !in_range) atomicOr(&ctr->err, kErrCoordRange);
          if (kFill) {
            rec[out + n] = make_uint4((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)vid | ((uint32_t)cloud << 12), (uint32_t)i);
            dest[out + n] = (uint32_t)shard_of(owner_hash(b[0], b[1], b[2]), nranks);
          }
          ++n;
        }
      }
    }
  }
  if (!kFill) counts[i] = n;
}

__global__ void vb_iota(uint32_t* __restrict__ a, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = i;
}

// counts[d] = records bound for rank d (dest sorted ascending): the first position of every destination by bisection
__global__ void vb_shard_dest_counts(const uint32_t* __restrict__ sorted_dest, uint32_t n, int nranks, uint32_t* __restrict__ counts) {
  const int d = threadIdx.x;
  if (d >= nranks) return;
  auto first_ge = [&](uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (sorted_dest[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  counts[d] = first_ge((uint32_t)d + 1u) - first_ge((uint32_t)d);
}

__global__ void vb_shard_gather(const uint4* __restrict__ rec, const uint32_t* __restrict__ order, uint32_t n, uint4* __restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) out[j] = rec[order ? order[j] : j];
}

// Received records: first-touch blocks enter the owner's directory (dir_insert never waits: the slot of a block inserted here
// is looked up by the NEXT kernel, as the count pass and the fill pass of the single-device call do — a find-or-insert that
// waits for another lane's slot met a circular wait between waves here, 64 records of a wave naming the same new block).
__global__ __launch_bounds__(256) void vb_shard_insert(const uint4* __restrict__ rec, uint32_t n, Directory dir, int rank, int nranks,
                                                       VCounters* __restrict__ ctr) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint4 r = rec[j];
  if (j > 0) {   // (consecutive records mostly name the same block: one insertion attempt per change)
    const uint4 q = rec[j - 1];
    if (q.x == r.x && q.y == r.y && (j & 63u) != 0u) return;
  }
  const unsigned long long key = (unsigned long long)r.x | ((unsigned long long)r.y << 32);
  const int x = (int)((key >> 42) & 0x1FFFFFu) - kCoordBias, y = (int)((key >> 21) & 0x1FFFFFu) - kCoordBias,
            z = (int)(key & 0x1FFFFFu) - kCoordBias;
  if (shard_of(owner_hash(x, y, z), nranks) != rank) atomicOr(&ctr->err, kErrDirectoryMiss);   // (a record sent to the wrong rank)
  else dir_insert(dir, x, y, z, &ctr->num_blocks, &ctr->err);
}

// ... -> voxel key in the owner's pool, sequence number, cloud.
__global__ __launch_bounds__(256) void vb_shard_translate(const uint4* __restrict__ rec, uint32_t n, Directory dir,
                                                          VCounters* __restrict__ ctr, uint32_t* __restrict__ vkey,
                                                          uint32_t* __restrict__ seq, uint32_t* __restrict__ cloud,
                                                          uint32_t* __restrict__ index) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint4 r = rec[j];
  const unsigned long long key = (unsigned long long)r.x | ((unsigned long long)r.y << 32);
  const int x = (int)((key >> 42) & 0x1FFFFFu) - kCoordBias, y = (int)((key >> 21) & 0x1FFFFFu) - kCoordBias,
            z = (int)(key & 0x1FFFFFu) - kCoordBias;
  const int slot = dir_find(dir, x, y, z);
  if (slot < 0) atomicOr(&ctr->err, kErrDirectoryMiss);
  vkey[j] = (slot < 0 ? 0u : (uint32_t)slot) * (uint32_t)kBlockVox + (r.z & 0xFFFu);
  seq[j] = r.w;
  if (cloud) {
    cloud[j] = r.z >> 12;
    index[j] = j;
  }
}

__global__ void vb_shard_permute(const uint32_t* __restrict__ vkey, const uint32_t* __restrict__ seq, const uint32_t* __restrict__ order,
                                 uint32_t n, uint32_t* __restrict__ keys_out, uint32_t* __restrict__ seq_out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t j = order[k];
  keys_out[k] = vkey[j];
  seq_out[k] = seq[j];
}

}  // namespace
}  // namespace

// ---- the three phases behind the entry points' argument checks (plvs_hip_tsdf_voxblox_shard_*, tsdf_voxblox.hip)

static int vb_shard_walk(plvs_tsdf_voxblox* h, const float* d_xyz, const int32_t* offsets, int nclouds, const float* d_Twc,
                         int64_t* send_counts, hipStream_t s) {
  const int N = std::max(1, h->P.shard_count), rank = N > 1 ? h->P.shard_rank : 0;
  PLVS_REQUIRE(N <= 64, "at most 64 ranks");
  for (int p = 0; p < N; ++p) send_counts[p] = 0;
  h->sv_V = 0;
  h->sv_phase = 1;
  h->sv_partitioned = false;
  int n = 0;
  int rc = check_offsets(offsets, nclouds, &n);
  if (rc != PLVS_OK) return rc;
  PLVS_REQUIRE((size_t)nclouds < ((size_t)1 << 20), "at most 2^20 clouds per call");
  if (n == 0) return PLVS_OK;
  PLVS_REQUIRE(d_xyz && d_Twc, "null device pointer");
  if (!h->h_sv_cnt) PLVS_HIP_TRY(hipHostMalloc((void**)&h->h_sv_cnt, 64 * sizeof(uint32_t)));
  rc = vb_call_head(h, offsets, nclouds, d_Twc, s);
  if (rc != PLVS_OK) return rc;
  PLVS_HIP_TRY(h->counts.reserve((size_t)n));
  PLVS_HIP_TRY(h->scratch.reserve(scan_scratch_words((size_t)n)));
  PLVS_HIP_TRY(h->sv_cnt.reserve(64));
  Params Pw = h->P;   // this rank's rays go through every block they cross
  Pw.shard_count = 1;
  Pw.shard_rank = 0;
  const dim3 rgrid(ceil_div((size_t)n, 256)), rblock(256);
  hipLaunchKernelGGL(vb_shard_ray_pass<false>, rgrid, rblock, 0, s, Pw, d_xyz, n, h->offsets.p, nclouds, h->poses.p, rank, N,
                     h->d_ctr, h->counts.p, (uint4*)nullptr, (uint32_t*)nullptr);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(exclusive_scan_u32(h->counts.p, h->counts.p, (size_t)n, &h->d_ctr->total_visits, h->scratch.p, s));
  rc = vb_read_counters(h, s);
  if (rc != PLVS_OK) return rc;
  if (h->h_ctr->err) return vb_fail(h, "shard_walk", h->h_ctr->err, false);
  const uint32_t V = h->h_ctr->total_visits;
  h->sv_V = V;
  if (V == 0) return PLVS_OK;
  PLVS_HIP_TRY(h->sv_rec.reserve(V));
  PLVS_HIP_TRY(h->sv_dest.reserve(V));
  hipLaunchKernelGGL(vb_shard_ray_pass<true>, rgrid, rblock, 0, s, Pw, d_xyz, n, h->offsets.p, nclouds, h->poses.p, rank, N,
                     h->d_ctr, h->counts.p, h->sv_rec.p, h->sv_dest.p);
  PLVS_KERNEL_CHECK();
  if (N == 1) {
    send_counts[0] = (int64_t)V;
    return PLVS_OK;
  }
  // stable partition by destination: one radix pass over (destination, record index)
  PLVS_HIP_TRY(h->sv_dest1.reserve(V));
  PLVS_HIP_TRY(h->sv_idx.reserve(V));
  PLVS_HIP_TRY(h->sv_idx1.reserve(V));
  PLVS_HIP_TRY(h->scratch.reserve(radix_scratch_words(V)));
  hipLaunchKernelGGL(vb_iota, dim3(ceil_div((size_t)V, 256)), dim3(256), 0, s, h->sv_idx.p, V);
  int bits = 1;
  while ((1 << bits) < N) ++bits;
  bool second = false;
  PLVS_HIP_TRY(radix_sort_pairs(h->sv_dest.p, h->sv_idx.p, h->sv_dest1.p, h->sv_idx1.p, V, 0, bits, h->scratch.p, s, &second));
  if (second) {   // (the gather of shard_pack reads sv_idx, the counts below sv_dest)
    std::swap(h->sv_dest, h->sv_dest1);
    std::swap(h->sv_idx, h->sv_idx1);
  }
  h->sv_partitioned = true;
  hipLaunchKernelGGL(vb_shard_dest_counts, dim3(1), dim3(64), 0, s, h->sv_dest.p, V, N, h->sv_cnt.p);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(hipMemcpyAsync(h->h_sv_cnt, h->sv_cnt.p, (size_t)N * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PLVS_HIP_TRY(hipStreamSynchronize(s));
  for (int p = 0; p < N; ++p) send_counts[p] = (int64_t)h->h_sv_cnt[p];
  return PLVS_OK;
}

static int vb_shard_pack(plvs_tsdf_voxblox* h, void* d_send, hipStream_t s) {
  h->sv_phase = 2;
  if (h->sv_V == 0) return PLVS_OK;
  PLVS_REQUIRE(d_send, "null send buffer");
  hipLaunchKernelGGL(vb_shard_gather, dim3(ceil_div((size_t)h->sv_V, 256)), dim3(256), 0, s, h->sv_rec.p,
                     h->sv_partitioned ? (const uint32_t*)h->sv_idx.p : (const uint32_t*)nullptr, h->sv_V, static_cast<uint4*>(d_send));
  PLVS_KERNEL_CHECK();
  return PLVS_OK;
}

static int vb_shard_apply(plvs_tsdf_voxblox* h, const void* d_recv, const int64_t* recv_counts, const float* d_xyz,
                          const uint8_t* d_rgba, const int32_t* offsets, int nclouds, const float* d_Twc, hipStream_t s) {
  h->sv_phase = 0;
  const int N = std::max(1, h->P.shard_count), rank = N > 1 ? h->P.shard_rank : 0;
  h->stats = plvs_tsdf_stats{};
  h->last_updated = 0;
  size_t total = 0;
  for (int p = 0; p < N; ++p) {
    PLVS_REQUIRE(recv_counts[p] >= 0, "negative receive count");
    total += (size_t)recv_counts[p];
  }
  PLVS_REQUIRE(total < 0xFFFFFFFFull, "receive buffer beyond the index range (split the batch)");
  const int n = nclouds > 0 ? offsets[nclouds] - offsets[0] : 0;
  h->stats.points = n;
  if (total == 0) return vb_publish_all(h, s);
  PLVS_REQUIRE(d_recv && d_xyz && d_rgba && d_Twc, "null device pointer");
  PLVS_REQUIRE((reinterpret_cast<uintptr_t>(d_rgba) & 3) == 0, "rgba must be 4-byte aligned");
  int rc = vb_halo_drop(h, s);   // new blocks go into the pool slots a meshing halo may still occupy
  if (rc != PLVS_OK) return rc;
  const uint32_t V = (uint32_t)total;
  rc = vb_call_head(h, offsets, nclouds, d_Twc, s);
  if (rc != PLVS_OK) return rc;
  rc = vb_reserve_visits(h, V);
  if (rc != PLVS_OK) return rc;
  const bool by_cloud = N > 1;   // (one source: the records are in sequence order already)
  if (by_cloud) {
    PLVS_HIP_TRY(h->sv_vkey.reserve(V));
    PLVS_HIP_TRY(h->sv_seq.reserve(V));
  }
  hipLaunchKernelGGL(vb_shard_insert, dim3(ceil_div((size_t)V, 256)), dim3(256), 0, s, static_cast<const uint4*>(d_recv), V, h->dir,
                     rank, N, h->d_ctr);
  hipLaunchKernelGGL(vb_shard_translate, dim3(ceil_div((size_t)V, 256)), dim3(256), 0, s, static_cast<const uint4*>(d_recv), V,
                     h->dir, h->d_ctr, by_cloud ? h->sv_vkey.p : h->keys0.p, by_cloud ? h->sv_seq.p : h->seq0.p,
                     by_cloud ? h->keys0.p : (uint32_t*)nullptr, by_cloud ? h->seq0.p : (uint32_t*)nullptr);
  PLVS_KERNEL_CHECK();
  rc = vb_read_counters(h, s);
  if (rc != PLVS_OK) return rc;
  if (h->h_ctr->err) return vb_fail(h, "shard_apply", h->h_ctr->err);
  const int before = h->num_blocks;
  h->num_blocks = h->h_ctr->num_blocks;
  const int published_lo = h->visible_blocks, published_hi = before;
  h->visible_blocks = h->num_blocks;
  h->stats.visits = V;
  h->stats.new_chunks = h->num_blocks - before;
  if (by_cloud) {   // (cloud, record index) -> the records in cloud order, each cloud's in its sender's (sequence) order
    bool second = false;
    int cbits = 1;
    while ((1ll << cbits) < (long long)nclouds) ++cbits;
    PLVS_HIP_TRY(radix_sort_pairs(h->keys0.p, h->seq0.p, h->keys1.p, h->seq1.p, V, 0, cbits, h->scratch.p, s, &second));
    const uint32_t* order = second ? h->seq1.p : h->seq0.p;
    uint32_t* k_out = second ? h->keys0.p : h->keys1.p;   // (the pair of buffers the sort has left free)
    uint32_t* q_out = second ? h->seq0.p : h->seq1.p;
    hipLaunchKernelGGL(vb_shard_permute, dim3(ceil_div((size_t)V, 256)), dim3(256), 0, s, h->sv_vkey.p, h->sv_seq.p, order, V, k_out, q_out);
    PLVS_KERNEL_CHECK();
    if (!second) {   // the permuted records sit in keys1 / seq1: make them the sort's input pair
      std::swap(h->keys0, h->keys1);
      std::swap(h->seq0, h->seq1);
    }
  }
  return vb_sort_and_fold(h, s, kSimple, V, d_xyz, nullptr, reinterpret_cast<const uint32_t*>(d_rgba), nclouds, published_lo,
                          published_hi, "shard_apply");
}
