// MergedTsdfIntegrator (Thirdparty/voxblox/src/integrator/tsdf_integrator.cc:361-470; integration method "merged", one
// thread): the points of a cloud that end in the same voxel are folded into one bundle, the bundles are cast as rays in the
// reference's integration order (the ordered pipeline, mode kMerged).  The kernels of the per-point part and of the fold, and
// the host-side bundling that replays the order of the reference's hash maps.
#pragma once
#include <unordered_map>
#include <vector>

#include "tsdf_voxblox_integrate.hpp"

namespace {

// MergedTsdfIntegrator::bundleRays, the per-point part (tsdf_integrator.cc:361-386): isPointValid -> kind (0 skipped,
// 1 normal, 2 clearing) and the voxel T_G_C * point_C ends in.  The grouping itself needs the reference's hash map and
// is done on the host (plvs_hip_tsdf_voxblox_integrate_merged).
__global__ __launch_bounds__(256) void vb_merge_keys(Params P, const float* __restrict__ xyz, int n,
                                                     const PoseRt* __restrict__ Twc, VCounters* __restrict__ ctr,
                                                     uint8_t* __restrict__ kind, int32_t* __restrict__ g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float px = xyz[3 * (size_t)i], py = xyz[3 * (size_t)i + 1], pz = xyz[3 * (size_t)i + 2];
  uint8_t k = 0;
  int v[3] = {0, 0, 0};
  if (!(isfinite(px) && isfinite(py) && isfinite(pz))) {
    atomicOr(&ctr->err, kErrNonFinite);
  } else {
    const float ray_distance = sqrtf(vsum3(px * px, py * py, pz * pz));
    if (ray_distance < P.min_ray) k = 0;
    else if (ray_distance > P.max_ray) k = P.allow_clear ? 2 : 0;
    else k = 1;
    if (k) {
      const PoseRt pose = load_pose(Twc, 0);
      float pG[3];
      quat_transform(pose, px, py, pz, pG);
      for (int c = 0; c < 3; ++c) v[c] = (int)floorf(pG[c] * P.voxel_size_inv + 1e-6f);
    }
  }
  kind[i] = k;
  g[3 * (size_t)i] = v[0];
  g[3 * (size_t)i + 1] = v[1];
  g[3 * (size_t)i + 2] = v[2];
}

// integrateVoxel's fold of a bundle's points into one (tsdf_integrator.cc:404-416), one thread per bundle: the
// recurrence is short (a handful of points per voxel) and sequential in float.
__global__ __launch_bounds__(256) void vb_merge_bundles(const float* __restrict__ xyz, const uint32_t* __restrict__ rgba,
                                                        const uint32_t* __restrict__ first, const uint32_t* __restrict__ pts,
                                                        const uint8_t* __restrict__ clr, int nb, float* __restrict__ mxyz,
                                                        uint32_t* __restrict__ mcol, float* __restrict__ mw) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  uint32_t colour = 0;   // Color()
  float m0 = 0.f, m1 = 0.f, m2 = 0.f, W = 0.f;
  const uint32_t end = clr[b] ? first[b] + 1u : first[b + 1];   // only the first point of a clearing bundle
  for (uint32_t j = first[b]; j < end; ++j) {
    const size_t p = pts[j];
    const float px = xyz[3 * p], py = xyz[3 * p + 1], pz = xyz[3 * p + 2];
    const float w = fabsf(pz) > 1e-6f ? 1.0f / (pz * pz) : 0.0f;   // getVoxelWeight
    const float tot = W + w;
    m0 = (m0 * W + px * w) / tot;
    m1 = (m1 * W + py * w) / tot;
    m2 = (m2 * W + pz * w) / tot;
    colour = blend_colours(colour, W, rgba[p], w);
    W += w;
  }
  mxyz[3 * (size_t)b] = m0;
  mxyz[3 * (size_t)b + 1] = m1;
  mxyz[3 * (size_t)b + 2] = m2;
  mcol[b] = colour;
  mw[b] = W;
}

}  // namespace

// plvs_hip_tsdf_voxblox_integrate_merged behind its argument checks.
static int vb_integrate_merged(plvs_tsdf_voxblox* h, const float* xyz, const uint8_t* rgba, int n, const float* Twc) {
  h->stats = plvs_tsdf_stats{};
  h->last_updated = 0;
  if (n == 0) return vb_empty_scan(h);   // (an empty cloud still publishes what a world cloud left waiting, as in the simple flavour)
  PLVS_REQUIRE(xyz && rgba, "null cloud pointer");
  hipStream_t s = nullptr;
  int rc = vb_stage_cloud(h, xyz, rgba, nullptr, n, Twc);
  if (rc != PLVS_OK) return rc;
  PLVS_HIP_TRY(h->mg_kind.reserve((size_t)n));
  PLVS_HIP_TRY(h->mg_g.reserve((size_t)n * 3));
  PLVS_HIP_TRY(hipMemsetAsync(&h->d_ctr->err, 0, sizeof(uint32_t), s));
  PLVS_HIP_TRY(h->poses.reserve(1));
  hipLaunchKernelGGL(vb_pose_prep, dim3(1), dim3(64), 0, s, h->st_Twc.p, 1, h->poses.p);
  hipLaunchKernelGGL(vb_merge_keys, dim3(ceil_div((size_t)n, 256)), dim3(256), 0, s, h->P, h->st_xyz.p, n, h->poses.p, h->d_ctr,
                     h->mg_kind.p, h->mg_g.p);
  PLVS_KERNEL_CHECK();
  std::vector<uint8_t> kind((size_t)n);
  std::vector<int32_t> g((size_t)n * 3);
  PLVS_HIP_TRY(hipMemcpy(kind.data(), h->mg_kind.p, (size_t)n, hipMemcpyDeviceToHost));
  PLVS_HIP_TRY(hipMemcpy(g.data(), h->mg_g.p, (size_t)n * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
  rc = vb_read_counters(h, s);
  if (rc != PLVS_OK) return rc;
  if (h->h_ctr->err & kErrNonFinite) {
    plvs::set_error("tsdf_voxblox integrate_merged: non-finite point in the cloud");
    return PLVS_ERR_INVALID_ARG;
  }
  // bundleRays (tsdf_integrator.cc:361-386): points in the mixed visiting order into voxel_map / clear_map.  The
  // integration order of the bundles is the iteration order of those maps (integrateVoxels, :448-470: begin(), ++it) —
  // AnyIndexHashMapType = std::unordered_map with AnyIndexHash (core/block_hash.h:15-34) — so the host fills the
  // same container with the same hash in the same sequence and walks it; nothing is computed here but that order.
  struct Key {
    int32_t v[3];
    bool operator==(const Key& o) const { return v[0] == o.v[0] && v[1] == o.v[1] && v[2] == o.v[2]; }
  };
  struct KeyHash {
    std::size_t operator()(const Key& k) const {
      return (static_cast<unsigned int>(k.v[0]) * std::size_t(73856093) ^ k.v[1] * std::size_t(19349663) ^
              k.v[2] * std::size_t(83492791));
    }
  };
  using BundleMap = std::unordered_map<Key, std::vector<uint32_t>, KeyHash>;
  BundleMap voxel_map, clear_map;
  for (uint32_t sq = 0; sq < (uint32_t)n; ++sq) {
    const uint32_t p = mixed_index(sq, (uint32_t)n);
    if (kind[p] == 0) continue;
    const Key k{{g[3 * (size_t)p], g[3 * (size_t)p + 1], g[3 * (size_t)p + 2]}};
    (kind[p] == 2 ? clear_map : voxel_map)[k].push_back(p);
  }
  const size_t nb = voxel_map.size() + clear_map.size();
  h->stats.points = n;
  if (nb == 0) {   // (every point skipped: nothing to cast, but the call still publishes waiting world-cloud blocks)
    const int rc0 = vb_empty_scan(h);
    h->stats.points = n;
    return rc0;
  }
  std::vector<uint32_t> first(nb + 1), pts;
  std::vector<uint8_t> clr(nb);
  pts.reserve((size_t)n);
  size_t b = 0;
  for (int pass = 0; pass < 2; ++pass)
    for (const auto& kv : (pass ? clear_map : voxel_map)) {
      first[b] = (uint32_t)pts.size();
      clr[b] = (uint8_t)pass;
      pts.insert(pts.end(), kv.second.begin(), kv.second.end());
      ++b;
    }
  first[nb] = (uint32_t)pts.size();
  PLVS_HIP_TRY(h->mg_first.reserve(nb + 1));
  PLVS_HIP_TRY(h->mg_pts.reserve(pts.size()));
  PLVS_HIP_TRY(h->mg_clr.reserve(nb));
  PLVS_HIP_TRY(h->mg_xyz.reserve(3 * nb));
  PLVS_HIP_TRY(h->mg_col.reserve(nb));
  PLVS_HIP_TRY(h->mg_w.reserve(nb));
  PLVS_HIP_TRY(hipMemcpy(h->mg_first.p, first.data(), (nb + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->mg_pts.p, pts.data(), pts.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  PLVS_HIP_TRY(hipMemcpy(h->mg_clr.p, clr.data(), nb, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(vb_merge_bundles, dim3(ceil_div(nb, 256)), dim3(256), 0, s, h->st_xyz.p, h->st_rgba.p, h->mg_first.p,
                     h->mg_pts.p, h->mg_clr.p, (int)nb, h->mg_xyz.p, h->mg_col.p, h->mg_w.p);
  PLVS_KERNEL_CHECK();
  const int32_t offsets[2] = {0, (int32_t)nb};
  rc = vb_integrate_impl(h, h->mg_xyz.p, reinterpret_cast<const uint8_t*>(h->mg_col.p), offsets, 1, h->st_Twc.p, nullptr, kMerged,
                         h->mg_w.p, h->mg_clr.p, 0);
  (void)hipDeviceSynchronize();
  h->stats.points = n;
  return rc;
}
