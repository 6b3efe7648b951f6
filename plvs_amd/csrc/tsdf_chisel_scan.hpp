// Projective depth + colour scan integrate (part of the tsdf_chisel.hip translation unit: it works on the map handle's
// internals, tsdf_chisel_handle.hpp, and on the carving path's frustum, tsdf_chisel_carve.hpp).
//
// Reference: PointCloudMapChisel::InsertDepthScanColor (src/PointCloudMapChisel.cc:134-189) ->
// ChiselServer::IntegrateLastDepthImage (ChiselServer.cpp:632-647) ->
// Chisel::IntegrateDepthScanColorWithOneCameraModelBGR (Chisel.h:198-258) ->
// ProjectionIntegrator::IntegrateColorWithOneCameraModelBGR (ProjectionIntegrator.h:189-269).
//
// Block-centric: every voxel centre of every chunk on the depth camera's frustum list (the list of the carving path:
// ChunkManager.cpp:241-271 + Frustum.cpp:41-79) is projected into the depth image.  A voxel within truncation +
// 2 sqrt(3) res of the measured surface takes the pixel's colour (while its colour weight is below 5) and
// DistVoxel::Integrate(surfaceDist, weight / (2 truncation)); with carving on, a known voxel further than truncation +
// carvingDist in front of the surface with sdf < 1e-5 is Reset().  Listed chunks the map does not have are created by
// the reference, integrated, and collected again when nothing updated them (Chisel.cpp:67-77).
//
// A voxel is touched at most once per scan, so there is no order inside a scan: one thread per voxel.  Whether a voxel
// takes the integrate branch depends on geometry and depth alone, never on the voxel — and a fresh voxel (weight 0)
// cannot be reset.  Hence
//   * scan_probe      decides, per (scan, listed chunk the map lacks), whether any voxel would be integrated; only
//                     those chunks get a pool slot.  What the reference creates and collects never exists here.  A
//                     chunk is rejected without testing its voxels only by scan_chunk_off_image's interval bound;
//   * scan_integrate  one thread per voxel of every chunk, voxel in registers, the K scans of a batch folded in call
//                     order.  A chunk first kept by scan k was "4096 fresh voxels" for the scans before it, which leave
//                     fresh voxels alone — so folding every scan over the chunk gives the reference's planes bit for bit.
// kfid is not written by this integrator.
#pragma once
#include "tsdf_chisel_handle.hpp"
#include "tsdf_chisel_halo.hpp"
#include "tsdf_chisel_carve.hpp"

namespace {

// Is the chunk on the frustum list of the camera?  (the test of carve_chunks, shared with the host replay of the
// chunk container)
__host__ __device__ __forceinline__ bool scan_lists_chunk(const Params& P, const CarveCamera& C, int x, int y, int z) {
  const int id[3] = {x, y, z};
  for (int k = 0; k < 3; ++k)
    if (id[k] < C.lo[k] || id[k] > C.hi[k]) return false;
  const float bmin[3] = {(float)(x * 16) * P.resolution, (float)(y * 16) * P.resolution, (float)(z * 16) * P.resolution};
  const float ext = 16.0f * P.resolution;
  for (int p = 0; p < 6; ++p) {
    float v[3];
    for (int k = 0; k < 3; ++k) v[k] = (C.plane_n[p][k] < 0.0f) ? bmin[k] : bmin[k] + ext;
    if (sum3(v[0] * C.plane_n[p][0], v[1] * C.plane_n[p][1], v[2] * C.plane_n[p][2]) + C.plane_d[p] > 0.0f) return true;
  }
  return false;
}

struct ScanHit {
  int kind;        // 0: the scan leaves the voxel alone, 1: integrate branch, 2: carving candidate
  int pixel;       // row * width + column of the depth (and colour) pixel
  float s, tau;    // surfaceDist, truncation
};

// ProjectionIntegrator.h:210-230, :253 for voxel i of chunk (x, y, z).
__device__ __forceinline__ ScanHit scan_voxel(const Params& P, const CarveCamera& C, const float* __restrict__ depth,
                                              int x, int y, int z, int i) {
  ScanHit r{0, 0, 0.0f, 0.0f};
  const int lx = i & 15, ly = (i >> 4) & 15, lz = i >> 8;
  const float cen[3] = {((float)lx * P.resolution + P.half_voxel) + (float)(x * 16) * P.resolution,
                        ((float)ly * P.resolution + P.half_voxel) + (float)(y * 16) * P.resolution,
                        ((float)lz * P.resolution + P.half_voxel) + (float)(z * 16) * P.resolution};
  const float d0 = cen[0] - C.t[0], d1 = cen[1] - C.t[1], d2 = cen[2] - C.t[2];
  float pc[3];
  for (int q = 0; q < 3; ++q) pc[q] = sum3(C.R[q] * d0, C.R[3 + q] * d1, C.R[6 + q] * d2);   // Rcw = R^T
  const float inv_z = 1.0f / pc[2];
  const float u = C.fx * pc[0] * inv_z + C.cx, v = C.fy * pc[1] * inv_z + C.cy;
  if (!(u >= 0 && v >= 0 && u < C.width && v < C.height) || pc[2] < 0) return r;
  const int col = (int)u, row = (int)v;
  if (col < 0 || col >= C.iwidth || row < 0 || (float)row >= C.height) return r;   // (cannot happen: the float test above)
  r.pixel = row * C.iwidth + col;
  const float d = depth[r.pixel];
  if (isnan(d)) return r;
  r.tau = (P.tq * d * d + P.tl * d + P.tc) * P.ts;   // QuadraticTruncator.h:49 — not floored here
  r.s = d - pc[2];
  if (fabsf(r.s) < r.tau + P.diag) r.kind = 1;
  else if (r.s > r.tau + C.carving_dist) r.kind = 2;
  return r;
}

// Can NO voxel centre of chunk (x, y, z) pass scan_voxel's "on the image and not behind the camera" test?  Conservative
// by monotonicity alone, no error budget: every operation of scan_voxel up to u and v is a correctly rounded float
// operation, and correct rounding is monotone in each operand (a <= b => RN(a op c) <= RN(b op c), reversed for a
// negative factor or a positive divisor).  So evaluating the SAME operations at the ends of the chunk's coordinate
// intervals bounds what any of its voxels computes:
//   cen_k in [cen_k(0), cen_k(15)], d_k = cen_k - t_k, R d_k by the sign of R, the 3-term sums, 1 / z for z > 0
//   (decreasing), (fx x) * (1 / z) between its four corner products, + cx.
// true only if zmax < 0, or z > 0 throughout and [umin, umax] or [vmin, vmax] misses [0, width) / [0, height).  A NaN
// anywhere compares false and answers "no".
__device__ __forceinline__ bool scan_chunk_off_image(const Params& P, const CarveCamera& C, int x, int y, int z) {
  const int id[3] = {x, y, z};
  float dlo[3], dhi[3];
  for (int k = 0; k < 3; ++k) {
    const float org = (float)(id[k] * 16) * P.resolution;
    dlo[k] = ((0.0f * P.resolution + P.half_voxel) + org) - C.t[k];
    dhi[k] = ((15.0f * P.resolution + P.half_voxel) + org) - C.t[k];
  }
  float lo[3], hi[3];
  for (int q = 0; q < 3; ++q) {
    float tl[3], th[3];
    for (int k = 0; k < 3; ++k) {
      const float r = C.R[3 * k + q], a = r * dlo[k], b = r * dhi[k];
      if (!(a == a) || !(b == b)) return false;
      tl[k] = a < b ? a : b;
      th[k] = a < b ? b : a;
    }
    lo[q] = sum3(tl[0], tl[1], tl[2]);
    hi[q] = sum3(th[0], th[1], th[2]);
  }
  if (hi[2] < 0.0f) return true;          // every voxel has pc[2] <= hi < 0
  if (!(lo[2] > 0.0f)) return false;      // the chunk straddles the camera plane: decided voxel by voxel
  const float il = 1.0f / hi[2], ih = 1.0f / lo[2];   // 1 / z over the chunk
  const float f[2] = {C.fx, C.fy}, c[2] = {C.cx, C.cy}, lim[2] = {C.width, C.height};
  for (int q = 0; q < 2; ++q) {
    const float a0 = f[q] * lo[q], a1 = f[q] * hi[q];
    const float al = a0 < a1 ? a0 : a1, ah = a0 < a1 ? a1 : a0;
    const float p[4] = {al * il, al * ih, ah * il, ah * ih};
    float ml = p[0], mh = p[0];
    for (int j = 0; j < 4; ++j) {
      if (!(p[j] == p[j])) return false;
      ml = p[j] < ml ? p[j] : ml;
      mh = p[j] > mh ? p[j] : mh;
    }
    if (!(a0 == a0) || !(a1 == a1)) return false;
    if (mh + c[q] < 0.0f || ml + c[q] >= lim[q]) return true;   // every voxel's u (v) lies in [ml + c, mh + c]
  }
  return false;
}

// One workgroup per (candidate chunk of the scan's id box, scan).  A listed chunk the map lacks gets a slot when one of
// its voxels takes the integrate branch.
__global__ __launch_bounds__(256) void scan_probe(Params P, const CarveCamera* __restrict__ cams,
                                                  const float* __restrict__ depth, size_t depth_stride, Directory dir,
                                                  Counters* __restrict__ ctr) {
  const CarveCamera& C = cams[blockIdx.y];
  const int ny = C.hi[1] - C.lo[1] + 1, nz = C.hi[2] - C.lo[2] + 1;
  const long long box = (long long)(C.hi[0] - C.lo[0] + 1) * ny * nz;
  if ((long long)blockIdx.x >= box) return;
  const int x = C.lo[0] + (int)(blockIdx.x / (unsigned)(ny * nz));
  const int rem = (int)(blockIdx.x % (unsigned)(ny * nz));
  const int y = C.lo[1] + rem / nz, z = C.lo[2] + rem % nz;
  if (!scan_lists_chunk(P, C, x, y, z)) return;
  if (dir_find(dir, x, y, z) >= 0) return;
  if (scan_chunk_off_image(P, C, x, y, z)) return;   // (uniform over the workgroup)
  const float* img = depth + (size_t)blockIdx.y * depth_stride;
  bool any = false;
  for (int part = 0; part < 16 && !any; ++part) {
    const ScanHit r = scan_voxel(P, C, img, x, y, z, (part << 8) | (int)threadIdx.x);
    any = __syncthreads_or(r.kind == 1) != 0;
  }
  if (any && threadIdx.x == 0) (void)dir_find_or_insert(dir, x, y, z, &ctr->num_chunks, &ctr->err);
}

// One thread per voxel: 16 workgroups of 256 per chunk, the four planes read once and written once per call.
// totals[0]: voxels integrated + voxels reset (u64).
__global__ __launch_bounds__(256) void scan_integrate(Params P, const CarveCamera* __restrict__ cams, int nscans,
                                                      const float* __restrict__ depth, size_t depth_stride,
                                                      const uint8_t* __restrict__ bgr, size_t bgr_stride, int channels,
                                                      int use_carving, const int32_t* __restrict__ slot_ids,
                                                      int num_chunks, float* __restrict__ sdf, float* __restrict__ weight,
                                                      uint32_t* __restrict__ vkfid, uint32_t* __restrict__ rgbw,
                                                      uint32_t* __restrict__ chunk_updated, Counters* __restrict__ ctr,
                                                      unsigned long long* __restrict__ totals) {
  const int slot = blockIdx.x >> 4;
  if (slot >= num_chunks) return;
  const int x = slot_ids[3 * slot], y = slot_ids[3 * slot + 1], z = slot_ids[3 * slot + 2];
  const int i = ((blockIdx.x & 15) << 8) | threadIdx.x;
  const size_t a = (size_t)slot * kChunkVox + (size_t)i;
  bool loaded = false;
  float v_sdf = 0.0f, v_w = 0.0f;
  uint32_t v_rgbw = 0u;
  bool sdf_dirty = false, rgbw_dirty = false, kfid_reset = false;
  uint32_t visits = 0u;
  for (int k = 0; k < nscans; ++k) {
    const CarveCamera& C = cams[k];
    if (!scan_lists_chunk(P, C, x, y, z)) continue;   // uniform over the workgroup
    if (!loaded) {
      v_sdf = sdf[a];
      v_w = weight[a];
      v_rgbw = rgbw[a];
      loaded = true;
    }
    const ScanHit r = scan_voxel(P, C, depth + (size_t)k * depth_stride, x, y, z, i);
    if (r.kind == 1) {
      if ((v_rgbw >> 24) < 5u) {   // ColorImage::AtBGR: blue, green, red = bytes 0, 1, 2 of the pixel
        const uint8_t* px = bgr + (size_t)k * bgr_stride + (size_t)r.pixel * (size_t)channels;
        colour_update(v_rgbw, px[2], px[1], px[0]);
        rgbw_dirty = true;
      }
      const float wu = P.weight / (2.0f * r.tau);   // ConstantWeighter.h:45
      dist_update(v_sdf, v_w, wu * r.s, wu);
      sdf_dirty = true;   // (kfid stays: a voxel reset earlier in the call keeps kfid 0)
      ++visits;
    } else if (r.kind == 2 && use_carving && v_w > 0 && (double)v_sdf < 1e-5) {
      v_sdf = 99999.0f;   // DistVoxel::Reset
      v_w = 0.0f;
      sdf_dirty = true;
      kfid_reset = true;
      ++visits;
    }
  }
  if (sdf_dirty) {
    sdf[a] = v_sdf;
    weight[a] = v_w;
  }
  if (rgbw_dirty) rgbw[a] = v_rgbw;
  if (kfid_reset) vkfid[a] = 0u;
  // ---- the chunk's updated flag, the call's counters
  __shared__ uint32_t s_visits, s_voxels;
  if (threadIdx.x == 0) { s_visits = 0u; s_voxels = 0u; }
  const bool updated = __syncthreads_or(visits != 0u) != 0;
  if (!updated) return;
  if (visits) {
    atomicAdd(&s_visits, visits);
    atomicAdd(&s_voxels, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    chunk_updated[slot] = 1u;
    atomicAdd(&totals[0], (unsigned long long)s_visits);
    atomicAdd(&ctr->num_heads, s_voxels);
  }
}

}  // namespace

// K scans resident in HBM; Twc on the host (12 floats per scan).  depth_stride / bgr_stride: elements / bytes between
// consecutive images; rows are dense.
static int scan_core(plvs_tsdf_chisel* h, const float* d_depth, size_t depth_stride, const uint8_t* d_bgr, size_t bgr_stride,
                     int channels, const plvs_scan_camera* cam, const float* Twc, int nscans, int use_carving,
                     float carving_dist, hipStream_t s) {
  {   // new chunks go into the pool slots a meshing halo may still occupy, and owned voxels change
    int rc = halo_drop(h, s);
    if (rc != PLVS_OK) return rc;
  }
  std::vector<CarveCamera> cams((size_t)nscans);
  unsigned box_max = 0;
  for (int k = 0; k < nscans; ++k) {
    CarveCamera& C = cams[(size_t)k];
    carve_frustum(h->P, Twc + 12 * (size_t)k, cam->near_plane, cam->far_plane, cam->fy, cam->cy, (float)cam->width,
                  (float)cam->height, &C);
    C.fx = cam->fx; C.fy = cam->fy; C.cx = cam->cx; C.cy = cam->cy;
    C.width = (float)cam->width; C.height = (float)cam->height; C.iwidth = cam->width;
    C.carving_dist = carving_dist;
    long long box = 1;
    for (int a = 0; a < 3; ++a) {
      PLVS_REQUIRE(C.lo[a] > -kCoordBias && C.hi[a] < kCoordBias && C.hi[a] >= C.lo[a] && C.hi[a] - C.lo[a] < 1024,
                   "the scan's frustum leaves the supported map extent (pose / near / far plane?)");
      box *= (long long)(C.hi[a] - C.lo[a] + 1);
    }
    PLVS_REQUIRE(box < (1ll << 30), "the scan's frustum spans too many chunks (far plane / resolution?)");
    box_max = std::max(box_max, (unsigned)box);
  }
  if (h->dfm) {   // the reference's container: every listed chunk the map lacks is inserted, in list order
    ChiselDeformState* st = h->dfm;
    const CarveCamera& C = cams[0];
    st->fresh.clear();
    for (int x = C.lo[0]; x <= C.hi[0]; ++x)
      for (int y = C.lo[1]; y <= C.hi[1]; ++y)
        for (int z = C.lo[2]; z <= C.hi[2]; ++z) {
          if (!scan_lists_chunk(h->P, C, x, y, z)) continue;
          const ChunkIdKey k{x, y, z};
          if (st->chunks.find(k) == st->chunks.end()) {
            st->chunks.insert(std::make_pair(k, true));   // CreateChunk, Chisel.h:220-224
            st->fresh.push_back(k);
          }
        }
  }
  static_assert(sizeof(CarveCamera) % sizeof(float) == 0, "cameras are uploaded through a float buffer");
  const size_t cam_words = (size_t)nscans * sizeof(CarveCamera) / sizeof(float);
  PLVS_HIP_TRY(h->st_Twc.reserve(cam_words));
  PLVS_HIP_TRY(hipMemcpyAsync(h->st_Twc.p, cams.data(), cam_words * sizeof(float), hipMemcpyHostToDevice, s));
  PLVS_HIP_TRY(hipStreamSynchronize(s));   // (`cams` is pageable and leaves scope)
  const CarveCamera* d_cams = reinterpret_cast<const CarveCamera*>(h->st_Twc.p);
  PLVS_HIP_TRY(h->counts.reserve(4));
  unsigned long long* d_totals = reinterpret_cast<unsigned long long*>(h->counts.p);
  PLVS_HIP_TRY(hipMemsetAsync(d_totals, 0, sizeof(unsigned long long), s));
  PLVS_HIP_TRY(hipMemsetAsync(&h->d_ctr->total_visits, 0, sizeof(uint32_t), s));
  PLVS_HIP_TRY(hipMemsetAsync(&h->d_ctr->err, 0, 5 * sizeof(uint32_t), s));
  hipLaunchKernelGGL(scan_probe, dim3(box_max, (unsigned)nscans), dim3(256), 0, s, h->P, d_cams, d_depth, depth_stride, h->dir,
                     h->d_ctr);
  PLVS_KERNEL_CHECK();
  int rc = read_counters(h, s);
  if (rc != PLVS_OK) return rc;
  if (h->h_ctr->err) {
    h->poisoned = true;
    plvs::set_error("tsdf_chisel integrate_scan: %s%s",
                    (h->h_ctr->err & kErrPoolFull) ? "chunk pool full (raise max_chunks) " : "",
                    (h->h_ctr->err & ~kErrPoolFull) ? "chunk directory error " : "");
    return PLVS_ERR_CAPACITY;
  }
  const int chunks_before = h->num_chunks;
  h->num_chunks = h->h_ctr->num_chunks;
  h->stats.new_chunks = h->num_chunks - chunks_before;
  if (h->num_chunks > 0) {
    PLVS_HIP_TRY(h->scratch.reserve((size_t)h->num_chunks));
    PLVS_HIP_TRY(h->updated.reserve((size_t)h->num_chunks + 1));
    PLVS_HIP_TRY(hipMemsetAsync(h->scratch.p, 0, (size_t)h->num_chunks * sizeof(uint32_t), s));
    hipLaunchKernelGGL(scan_integrate, dim3((unsigned)h->num_chunks * 16u), dim3(256), 0, s, h->P, d_cams, nscans, d_depth,
                       depth_stride, d_bgr, bgr_stride, channels, use_carving, h->dir.slot_ids, h->num_chunks, h->sdf, h->weight,
                       h->kfid, h->rgbw, h->scratch.p, h->d_ctr, d_totals);
    hipLaunchKernelGGL(carve_collect, dim3(ceil_div((size_t)h->num_chunks, 256)), dim3(256), 0, s, h->scratch.p, h->num_chunks,
                       h->updated.p, h->d_ctr);
    PLVS_KERNEL_CHECK();
    unsigned long long visits = 0;
    PLVS_HIP_TRY(hipMemcpyAsync(&visits, d_totals, sizeof(visits), hipMemcpyDeviceToHost, s));
    rc = read_counters(h, s);
    if (rc != PLVS_OK) return rc;
    h->last_updated = h->h_ctr->num_updated;
    h->stats.visits = (int64_t)visits;
    h->stats.updated_chunks = (int32_t)h->last_updated;
    h->stats.voxels = (int32_t)h->h_ctr->num_heads;
  }
  if (h->dfm) return deform_track_end(h, s);   // GarbageCollect (Chisel.cpp:67-77): erases in list order
  return PLVS_OK;
}

static int scan_check(plvs_tsdf_chisel* h, const plvs_scan_camera* cam, int channels) {
  PLVS_REQUIRE(h && cam, "null argument");
  PLVS_REQUIRE(!h->poisoned, "handle is in a failed state (clear it)");
  PLVS_REQUIRE(h->prm.order_free == 0, "the scan integrate is not available on an order-free map");
  PLVS_REQUIRE(h->P.shard_count <= 1, "the scan integrate is not available on a sharded map");
  PLVS_REQUIRE(cam->width > 0 && cam->height > 0 && (long long)cam->width * cam->height < (1ll << 28), "bad image size");
  PLVS_REQUIRE(channels == 3 || channels == 4, "the colour image has 3 (BGR) or 4 (BGRA) channels");
  PLVS_REQUIRE(cam->far_plane > cam->near_plane && cam->near_plane >= 0.0f, "bad near / far plane");
  return PLVS_OK;
}

extern "C" {

// Chisel::IntegrateDepthScanColorWithOneCameraModelBGR (Chisel.h:198-258) for K scans in call order.
int plvs_hip_tsdf_chisel_integrate_scans_dev(plvs_tsdf_chisel* h, const float* d_depth, const uint8_t* d_bgr, int channels,
                                             const plvs_scan_camera* camera, const float* d_Twc, int nscans, int use_carving,
                                             float carving_dist, void* stream) {
  PLVS_FLUSH_QUEUE(h);
  int rc = scan_check(h, camera, channels);
  if (rc != PLVS_OK) return rc;
  PLVS_REQUIRE(nscans >= 0, "bad scan count");
  h->stats = plvs_tsdf_stats{};
  h->last_updated = 0;
  if (nscans == 0) return PLVS_OK;
  PLVS_REQUIRE(d_depth && d_Twc, "null device pointer");
  PLVS_REQUIRE(d_bgr, "a colour image is required (the depth-only IntegrateDepthScan is not provided)");
  PLVS_REQUIRE(h->dfm == nullptr || nscans == 1,
               "a map with deform enabled takes one scan per call (the reference's chunk order is per call)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<float> Twc(12 * (size_t)nscans);
  PLVS_HIP_TRY(hipMemcpyAsync(Twc.data(), d_Twc, Twc.size() * sizeof(float), hipMemcpyDeviceToHost, s));
  PLVS_HIP_TRY(hipStreamSynchronize(s));
  const size_t npix = (size_t)camera->width * (size_t)camera->height;
  return scan_core(h, d_depth, npix, d_bgr, npix * (size_t)channels, channels, camera, Twc.data(), nscans, use_carving,
                   carving_dist, s);
}

// PointCloudMapChisel::InsertDepthScanColor's shape (src/PointCloudMapChisel.cc:134-189): host images with row pitches.
int plvs_hip_tsdf_chisel_integrate_scan(plvs_tsdf_chisel* h, const float* depth, int depth_pitch_bytes, const uint8_t* bgr,
                                        int bgr_pitch_bytes, int channels, const plvs_scan_camera* camera, const float* Twc,
                                        int use_carving, float carving_dist) {
  PLVS_FLUSH_QUEUE(h);
  int rc = scan_check(h, camera, channels);
  if (rc != PLVS_OK) return rc;
  PLVS_REQUIRE(depth && Twc, "null argument");
  PLVS_REQUIRE(bgr, "a colour image is required (the depth-only IntegrateDepthScan is not provided)");
  const size_t w = (size_t)camera->width, hgt = (size_t)camera->height;
  PLVS_REQUIRE(depth_pitch_bytes >= (int)(w * sizeof(float)) && depth_pitch_bytes % (int)sizeof(float) == 0, "bad depth pitch");
  PLVS_REQUIRE(bgr_pitch_bytes >= (int)(w * (size_t)channels), "bad colour pitch");
  h->stats = plvs_tsdf_stats{};
  h->last_updated = 0;
  PLVS_HIP_TRY(h->st_xyz.reserve(w * hgt));
  PLVS_HIP_TRY(h->st_rgb.reserve(w * hgt * (size_t)channels));
  PLVS_HIP_TRY(hipMemcpy2D(h->st_xyz.p, w * sizeof(float), depth, (size_t)depth_pitch_bytes, w * sizeof(float), hgt,
                           hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy2D(h->st_rgb.p, w * (size_t)channels, bgr, (size_t)bgr_pitch_bytes, w * (size_t)channels, hgt,
                           hipMemcpyHostToDevice));
  rc = scan_core(h, h->st_xyz.p, w * hgt, h->st_rgb.p, w * hgt * (size_t)channels, channels, camera, Twc, 1, use_carving,
                 carving_dist, nullptr);
  if (rc != PLVS_OK) return rc;
  PLVS_HIP_TRY(hipDeviceSynchronize());
  return PLVS_OK;
}

}  // extern "C"
