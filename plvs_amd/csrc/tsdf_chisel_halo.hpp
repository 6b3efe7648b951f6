// Halo of a sharded map: ghost copies of other ranks' chunks, in the pool slots past num_chunks, so that meshing can read
// across the shard boundary.  A rank looks up and exports the chunks it is asked for (halo_lookup, halo_export), the asker
// imports them behind its own (halo_import); every call that adds chunks drops the ghosts first (halo_drop).
#pragma once
#include "tsdf_chisel_handle.hpp"

namespace {

constexpr int kHaloWords = 4 * kChunkVox;   // a chunk on the wire: sdf, weight, kfid, rgbw planes

// Which of the requested chunks this rank has.
__global__ void halo_lookup_chunks(Directory dir, const int32_t* __restrict__ ids, int n, uint32_t* __restrict__ found) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) found[i] = dir_find(dir, ids[3 * i], ids[3 * i + 1], ids[3 * i + 2]) >= 0 ? 1u : 0u;
}

// row[i] = number of found chunks before request i (one workgroup; request lists are a few thousand long).
__global__ __launch_bounds__(1024) void halo_rows(const uint32_t* __restrict__ found, int n, uint32_t* __restrict__ row) {
  __shared__ uint32_t s_part[1024];
  const int per = (n + 1023) / 1024;
  const int lo = min((int)threadIdx.x * per, n), hi = min(lo + per, n);
  uint32_t sum = 0;
  for (int i = lo; i < hi; ++i) sum += found[i] ? 1u : 0u;
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const uint32_t add = threadIdx.x >= (unsigned)d ? s_part[threadIdx.x - d] : 0u;
    __syncthreads();
    s_part[threadIdx.x] += add;
    __syncthreads();
  }
  uint32_t run = s_part[threadIdx.x] - sum;
  for (int i = lo; i < hi; ++i) {
    row[i] = run;
    run += found[i] ? 1u : 0u;
  }
}

// The found chunks' planes, one payload row (kHaloWords) each, in request order.
__global__ __launch_bounds__(256) void halo_export_chunks(Directory dir, const float* __restrict__ sdf,
                                                          const float* __restrict__ weight, const uint32_t* __restrict__ kfid,
                                                          const uint32_t* __restrict__ rgbw, const int32_t* __restrict__ ids,
                                                          const uint32_t* __restrict__ found, const uint32_t* __restrict__ row,
                                                          uint32_t* __restrict__ payload) {
  const int i = blockIdx.x;
  if (!found[i]) return;
  __shared__ int s_slot;
  if (threadIdx.x == 0) s_slot = dir_find(dir, ids[3 * i], ids[3 * i + 1], ids[3 * i + 2]);
  __syncthreads();
  const int slot = s_slot;
  if (slot < 0) return;
  const size_t src = (size_t)slot * kChunkVox;
  uint4* dst = reinterpret_cast<uint4*>(payload + (size_t)row[i] * kHaloWords);
  const uint4* p0 = reinterpret_cast<const uint4*>(sdf + src);
  const uint4* p1 = reinterpret_cast<const uint4*>(weight + src);
  const uint4* p2 = reinterpret_cast<const uint4*>(kfid + src);
  const uint4* p3 = reinterpret_cast<const uint4*>(rgbw + src);
  for (int v = threadIdx.x; v < kChunkVox / 4; v += 256) {
    dst[v] = p0[v];
    dst[kChunkVox / 4 + v] = p1[v];
    dst[2 * (kChunkVox / 4) + v] = p2[v];
    dst[3 * (kChunkVox / 4) + v] = p3[v];
  }
}

// id -> ghost slot (base + its payload row), or kGhostAbsent for a chunk its owner does not have; an id already
// present keeps its entry.
__global__ void halo_insert(Directory g, const int32_t* __restrict__ ids, const uint32_t* __restrict__ found,
                            const uint32_t* __restrict__ row, int n, int base, uint32_t* __restrict__ err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = ids[3 * i], y = ids[3 * i + 1], z = ids[3 * i + 2];
  unsigned long long key;
  if (!pack_block(x, y, z, &key)) {
    atomicOr(err, kErrCoordRange);
    return;
  }
  uint32_t hsh = dir_hash(x, y, z, g.mask);
  for (uint32_t probe = 0; probe <= g.mask; ++probe) {
    unsigned long long cur = g.keys[hsh];
    if (cur == key) return;
    if (cur == kEmptyKey) {
      cur = atomicCAS(&g.keys[hsh], kEmptyKey, key);
      if (cur == kEmptyKey) {
        g.slots[hsh] = found[i] ? base + (int)row[i] : plvs::tsdf::kGhostAbsent;
        return;
      }
      if (cur == key) return;
    }
    hsh = (hsh + 1) & g.mask;
  }
  atomicOr(err, kErrPoolFull);
}

__global__ __launch_bounds__(256) void halo_import_chunks(float* __restrict__ sdf, float* __restrict__ weight,
                                                          uint32_t* __restrict__ kfid, uint32_t* __restrict__ rgbw,
                                                          const uint32_t* __restrict__ found, const uint32_t* __restrict__ row,
                                                          const uint32_t* __restrict__ payload, int base) {
  const int i = blockIdx.x;
  if (!found[i]) return;
  const size_t dst = (size_t)(base + (int)row[i]) * kChunkVox;
  const uint4* src = reinterpret_cast<const uint4*>(payload + (size_t)row[i] * kHaloWords);
  uint4* p0 = reinterpret_cast<uint4*>(sdf + dst);
  uint4* p1 = reinterpret_cast<uint4*>(weight + dst);
  uint4* p2 = reinterpret_cast<uint4*>(kfid + dst);
  uint4* p3 = reinterpret_cast<uint4*>(rgbw + dst);
  for (int v = threadIdx.x; v < kChunkVox / 4; v += 256) {
    p0[v] = src[v];
    p1[v] = src[kChunkVox / 4 + v];
    p2[v] = src[2 * (kChunkVox / 4) + v];
    p3[v] = src[3 * (kChunkVox / 4) + v];
  }
}

// Ghost slots back to the state of a never-used pool slot (clear() leaves sdf 99999, everything else 0).
__global__ __launch_bounds__(256) void halo_reset_slots(float* __restrict__ sdf, float* __restrict__ weight,
                                                        uint32_t* __restrict__ kfid, uint32_t* __restrict__ rgbw, int base) {
  const size_t at = (size_t)(base + blockIdx.x) * kChunkVox;
  for (int v = threadIdx.x; v < kChunkVox; v += 256) {
    sdf[at + v] = 99999.0f;
    weight[at + v] = 0.f;
    kfid[at + v] = 0u;
    rgbw[at + v] = 0u;
  }
}

}  // namespace

// Drops the ghosts (the integrate calls allocate new chunks in the slots they occupy).
static int halo_drop(plvs_tsdf_chisel* h, hipStream_t s) {
  if (h->ghost_entries == 0) return PLVS_OK;
  if (h->ghost_count > 0) {
    hipLaunchKernelGGL(halo_reset_slots, dim3((unsigned)h->ghost_count), dim3(256), 0, s, h->sdf, h->weight, h->kfid, h->rgbw,
                       h->num_chunks);
    PLVS_KERNEL_CHECK();
  }
  PLVS_HIP_TRY(hipMemsetAsync(h->gdir.keys, 0xFF, ((size_t)h->gdir.mask + 1) * sizeof(unsigned long long), s));
  h->ghost_count = 0;
  h->ghost_entries = 0;
  return PLVS_OK;
}

extern "C" {

int plvs_hip_tsdf_chisel_halo_missing(plvs_tsdf_chisel* h, int32_t* ids_xyz, int cap, int* n) {
  PLVS_REQUIRE(h && n, "null argument");
  *n = 0;
  if (h->miss_count == nullptr) return PLVS_OK;
  uint32_t cnt = 0;
  PLVS_HIP_TRY(hipMemcpy(&cnt, h->miss_count, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (cnt > h->miss_cap) {
    plvs::set_error("halo_missing: %u missing chunks exceed the list capacity %u", cnt, h->miss_cap);
    return PLVS_ERR_CAPACITY;
  }
  *n = (int)cnt;
  if (cnt == 0) return PLVS_OK;
  if ((int)cnt > cap) return PLVS_ERR_CAPACITY;
  PLVS_REQUIRE(ids_xyz, "null output");
  PLVS_HIP_TRY(hipMemcpy(ids_xyz, h->miss_ids, (size_t)cnt * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_halo_lookup(plvs_tsdf_chisel* h, const int32_t* d_ids_xyz, int n, uint32_t* d_found, void* stream) {
  PLVS_REQUIRE(h && !h->poisoned, "unusable handle");
  PLVS_REQUIRE(n >= 0, "negative size");
  if (n == 0) return PLVS_OK;
  PLVS_REQUIRE(d_ids_xyz && d_found, "null argument");
  hipLaunchKernelGGL(halo_lookup_chunks, dim3(ceil_div((size_t)n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), h->dir,
                     d_ids_xyz, n, d_found);
  PLVS_KERNEL_CHECK();
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_halo_export(plvs_tsdf_chisel* h, const int32_t* d_ids_xyz, const uint32_t* d_found, int n,
                                     uint32_t* d_payload, void* stream) {
  PLVS_REQUIRE(h && !h->poisoned, "unusable handle");
  PLVS_REQUIRE(n >= 0, "negative size");
  if (n == 0 || d_payload == nullptr) return PLVS_OK;   // (no payload buffer: the caller saw no flag set)
  PLVS_REQUIRE(d_ids_xyz && d_found, "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  PLVS_HIP_TRY(h->halo_row.reserve((size_t)n));
  hipLaunchKernelGGL(halo_rows, dim3(1), dim3(1024), 0, s, d_found, n, h->halo_row.p);
  hipLaunchKernelGGL(halo_export_chunks, dim3((unsigned)n), dim3(256), 0, s, h->dir, h->sdf, h->weight, h->kfid, h->rgbw,
                     d_ids_xyz, d_found, h->halo_row.p, d_payload);
  PLVS_KERNEL_CHECK();
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_halo_import(plvs_tsdf_chisel* h, const int32_t* d_ids_xyz, const uint32_t* d_found,
                                     const uint32_t* d_payload, int n, int nfound, void* stream) {
  PLVS_REQUIRE(h && !h->poisoned, "unusable handle");
  PLVS_REQUIRE(n >= 0 && nfound >= 0 && nfound <= n, "bad sizes");
  if (n == 0) return PLVS_OK;
  PLVS_REQUIRE(d_ids_xyz && d_found && (nfound == 0 || d_payload), "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((long long)h->num_chunks + h->ghost_count + nfound > (long long)h->prm.max_chunks) {
    plvs::set_error("halo_import: %d own + %d ghost + %d new chunks exceed the pool (%d)", h->num_chunks, h->ghost_count, nfound,
                    h->prm.max_chunks);
    return PLVS_ERR_CAPACITY;
  }
  if (h->gdir.keys == nullptr) {
    // entries are foreign chunks that exist (at most the pool's worth) and ids that exist nowhere (the colour look-up's
    // reach: thousands per call), kept until the next integrate call: twice the miss set's table
    size_t cap = 2 * std::max<size_t>((size_t)h->miss_mask + 1, (size_t)1 << 19);
    while (cap < 4 * (size_t)h->prm.max_chunks) cap <<= 1;
    // (both tables or neither: a half-built ghost directory would be taken for a complete one by the next call)
    unsigned long long* gkeys = nullptr;
    int32_t* gslots = nullptr;
    PLVS_HIP_TRY(hipMalloc(&gkeys, cap * sizeof(unsigned long long)));
    {
      const hipError_t e = hipMalloc(&gslots, cap * sizeof(int32_t));
      if (e != hipSuccess) {
        (void)hipFree(gkeys);
        PLVS_HIP_TRY(e);
      }
    }
    h->gdir.keys = gkeys;
    h->gdir.slots = gslots;
    h->gdir.slot_ids = nullptr;
    h->gdir.mask = (uint32_t)(cap - 1);
    h->gdir.max_blocks = h->prm.max_chunks;
    PLVS_HIP_TRY(hipMemsetAsync(h->gdir.keys, 0xFF, cap * sizeof(unsigned long long), s));
  }
  if ((size_t)h->ghost_entries + (size_t)n > ((size_t)h->gdir.mask + 1) / 2) {
    plvs::set_error("halo_import: %lld + %d entries exceed the ghost directory (halo_clear drops them)", h->ghost_entries, n);
    return PLVS_ERR_CAPACITY;
  }
  const int base = h->num_chunks + h->ghost_count;
  PLVS_HIP_TRY(h->halo_row.reserve((size_t)n));
  hipLaunchKernelGGL(halo_rows, dim3(1), dim3(1024), 0, s, d_found, n, h->halo_row.p);
  hipLaunchKernelGGL(halo_insert, dim3(ceil_div((size_t)n, 256)), dim3(256), 0, s, h->gdir, d_ids_xyz, d_found, h->halo_row.p, n,
                     base, &h->d_ctr->err);
  if (nfound > 0)
    hipLaunchKernelGGL(halo_import_chunks, dim3((unsigned)n), dim3(256), 0, s, h->sdf, h->weight, h->kfid, h->rgbw, d_found,
                       h->halo_row.p, d_payload, base);
  PLVS_KERNEL_CHECK();
  h->ghost_count += nfound;
  h->ghost_entries += n;
  return PLVS_OK;
}

int plvs_hip_tsdf_chisel_halo_clear(plvs_tsdf_chisel* h) {
  PLVS_REQUIRE(h, "null handle");
  int rc = halo_drop(h, nullptr);
  if (rc != PLVS_OK) return rc;
  PLVS_HIP_TRY(hipStreamSynchronize(nullptr));
  return PLVS_OK;
}

}  // extern "C"
