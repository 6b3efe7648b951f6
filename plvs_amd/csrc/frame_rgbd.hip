// What makes a frame RGB-D: Frame::ComputeStereoFromRGBD (reference src/Frame.cc:2251-2279) and
// Frame::ComputeStereoLinesFromRGBD (:2434-2674 with computeLocalMinDepth / computeLocalMinMaxDepth, :2311-2370, the live
// CHECK_RGBD_ENDPOINTS_DEPTH_CONSISTENCY path), Frame::ComputeSceneMedianDepth (:2730-2751) and the RGB-D constructor
// (:401-600) as one call over the entries of frame.hip / frame_glue.hip.  Both association loops run in ONE launch: the
// first ceil(n / 256) workgroups take a key point per thread, the others a line per thread; the depth image stays where it
// is (HBM, pitch in floats) and a thread reads 1 or 27 of its pixels.
//
// Arithmetic: the reference's own sequence.  f32 where it computes in float (the back-projection, the Emax / Smax scale,
// mbf / d), f64 where it builds Eigen::Vector3d from f32 differences: cross by the plain formula, sums of three as
// c0 + (c1 + c2) (Eigen's unrolled reduction), norm = sqrt, every cross.norm() / norm() quotient narrowed to f32.  The
// translation unit is built with -ffp-contract=off (nothing fuses), and `/`, sqrt on f32 and f64 are the compiler's
// correctly rounded sequences (no fast-math, no approximate builtins) — the forms plvs_hip_selftest_walk_math holds the
// TSDF walk's shortcuts to.  The gain over the host loops is the depth image that no longer has to exist on the host and
// the round trip that goes with it, not the arithmetic.
#include <cfloat>
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "frame_geom.hpp"

namespace {

constexpr int kGridCells = 64 * 48;   // FRAME_GRID_COLS x FRAME_GRID_ROWS, include/Frame.h:67-68

struct RgbdParams {
  int width, height, pitch;          // the depth image, pitch in floats
  float cx, cy, invfx, invfy;        // Frame::cx, cy, invfx = 1.0f / fx, invfy (:458-459)
  float mbf;
  float min_line_length_3d;          // Frame::skMinLineLength3D
  float cos_view_z_angle_max;        // Frame::kCosViewZAngleMax, computed on the host
};

using plvs::V3;
using plvs::v3;
using plvs::cross;
using plvs::norm;
using plvs::dot;
using plvs::normalized;   // Eigen::Vector3d in the reference's evaluation order: frame_geom.hpp, shared with frame_stereo.hip

// float -> int as `const int&` binds it (truncation), kept inside [-2, limit + 1]: the 3 x 3 window of anything beyond
// misses the image either way, and u + du cannot overflow.
__device__ __forceinline__ int pixel_of(float f, int limit) {
  const int i = (int)f;
  return i < -2 ? -2 : (i > limit + 1 ? limit + 1 : i);
}

// computeLocalMinMaxDepth (:2338-2370) with delta 1: min and max of the finite values > 0 of the clipped 3 x 3 window, 0
// when there is none; computeLocalMinDepth (:2311-2336) is its first half.
__device__ __forceinline__ void local_min_max(const RgbdParams& P, const float* __restrict__ depth, float fu, float fv, float* min_out,
                                              float* max_out) {
  const int u = pixel_of(fu, P.width), v = pixel_of(fv, P.height);
  float mn = FLT_MAX, mx = 0.0f;
  for (int du = -1; du <= 1; ++du)
    for (int dv = -1; dv <= 1; ++dv) {
      const int ou = u + du, ov = v + dv;
      if (ou >= 0 && ou < P.width && ov >= 0 && ov < P.height) {
        const float val = depth[(size_t)ov * (size_t)P.pitch + (size_t)ou];
        if (isfinite(val) && val > 0.0f) {
          if (mn > val) mn = val;
          if (mx < val) mx = val;
        }
      }
    }
  *min_out = mn < FLT_MAX ? mn : 0.0f;
  *max_out = mx > 0.0f ? mx : 0.0f;
}

// One line of Frame::ComputeStereoLinesFromRGBD.  in8 = uS vS uE vE of mvKeyLines[i], then of mvKeyLinesUn[i].
__device__ __forceinline__ void associate_line(const RgbdParams& P, const float* __restrict__ depth, const float* __restrict__ in8,
                                               float* out4) {
  const float kMaxMisalignment = 0.03f;   // Frame::kLinePointsMaxMisalignment (:107)
  const float uS = in8[0], vS = in8[1], uE = in8[2], vE = in8[3];
  const float uSU = in8[4], vSU = in8[5], uEU = in8[6], vEU = in8[7];
  const float vM = 0.5f * (vS + vE), uM = 0.5f * (uS + uE);   // (0.5 * float in double, narrowed: the same halving)
  const float vMU = 0.5f * (vSU + vEU), uMU = 0.5f * (uSU + uEU);
  float dS, dSmax, dE, dEmax, dM, unused;
  local_min_max(P, depth, uS, vS, &dS, &dSmax);
  local_min_max(P, depth, uE, vE, &dE, &dEmax);
  local_min_max(P, depth, uM, vM, &dM, &unused);
  if (dS > 0.0f && dE > 0.0f) {
    float xS = (uSU - P.cx) * dS * P.invfx, yS = (vSU - P.cy) * dS * P.invfy;
    float xE = (uEU - P.cx) * dE * P.invfx, yE = (vEU - P.cy) * dE * P.invfy;
    V3 lineES = v3(xS - xE, yS - yE, dS - dE);
    if (dM > 0.0f) {
      const float xM = (uMU - P.cx) * dM * P.invfx, yM = (vMU - P.cy) * dM * P.invfy;
      V3 lineMS = v3(xS - xM, yS - yM, dS - dM);
      V3 lineEM = v3(xM - xE, yM - yE, dM - dE);
      float distM_SE = (float)(norm(cross(lineMS, lineEM)) / norm(lineES));
      if (distM_SE > kMaxMisalignment) {
        if (dEmax > 0.0f) {   // E -> Emax?
          const float scale = dEmax / dE;
          const float xEmax = xE * scale, yEmax = yE * scale;
          const V3 lineEmaxM = v3(xM - xEmax, yM - yEmax, dM - dEmax);
          const V3 lineEmaxS = v3(xS - xEmax, yS - yEmax, dS - dEmax);
          const float d2 = (float)(norm(cross(lineMS, lineEmaxM)) / norm(lineEmaxS));
          if (d2 < kMaxMisalignment && d2 < distM_SE) {
            xE = xEmax; yE = yEmax; dE = dEmax;
            lineEM = lineEmaxM;
            lineES = lineEmaxS;
            distM_SE = d2;
          }
        }
        if (dSmax > 0.0f) {   // S -> Smax? (against the E the step above left)
          const float scale = dSmax / dS;
          const float xSmax = xS * scale, ySmax = yS * scale;
          const V3 lineMSmax = v3(xSmax - xM, ySmax - yM, dSmax - dM);
          const V3 lineESmax = v3(xSmax - xE, ySmax - yE, dSmax - dE);
          const float d2 = (float)(norm(cross(lineMSmax, lineEM)) / norm(lineESmax));
          if (d2 < kMaxMisalignment && d2 < distM_SE) {
            xS = xSmax; yS = ySmax; dS = dSmax;
            lineMS = lineMSmax;
            lineES = lineESmax;
            distM_SE = d2;
          }
        }
      }
      if (distM_SE > kMaxMisalignment) dS = dE = -1.0f;
    }
    if (norm(lineES) < (double)P.min_line_length_3d) dS = dE = -1.0f;   // (also after a rejection, as there)
    if (dS > 0.0f && dE > 0.0f) {
      const V3 camRay = normalized(v3(xS, yS, dS));
      const V3 dir = normalized(v3(xS - xE, yS - yE, dS - dE));
      const float cosViewAngle = fabsf((float)dot(camRay, dir));
      if (cosViewAngle > P.cos_view_z_angle_max) dS = dE = -1.0f;
    }
  }
  if (dS > 0.0f && isfinite(dS) && dE > 0.0f && isfinite(dE)) {
    out4[0] = uSU - P.mbf / dS;
    out4[1] = dS;
    out4[2] = uEU - P.mbf / dE;
    out4[3] = dE;
  } else {
    out4[0] = out4[1] = out4[2] = out4[3] = -1.0f;
  }
}

// points: n x (u, v of mvKeys[i], u of mvKeysUn[i]) -> point_out: n x (uRight, depth); lines: n_lines x 8 (associate_line)
// -> line_out: n_lines x (uRightStart, depthStart, uRightEnd, depthEnd).
__global__ __launch_bounds__(256) void rgbd_associate_kernel(RgbdParams P, const float* __restrict__ depth, const float* __restrict__ points,
                                                             int n, int point_blocks, const float* __restrict__ lines, int n_lines,
                                                             float* __restrict__ point_out, float* __restrict__ line_out) {
  if ((int)blockIdx.x < point_blocks) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    // imDepth.at<float>(v, u): both floats truncated; a key point outside the image (undefined there) reads nothing
    const int u = pixel_of(points[3 * i], P.width), v = pixel_of(points[3 * i + 1], P.height);
    float ur = -1.0f, z = -1.0f;
    if (u >= 0 && u < P.width && v >= 0 && v < P.height) {
      const float d = depth[(size_t)v * (size_t)P.pitch + (size_t)u];
      if (d > 0.0f) {
        z = d;
        ur = points[3 * i + 2] - P.mbf / d;
      }
    }
    point_out[2 * i] = ur;
    point_out[2 * i + 1] = z;
  } else {
    const int i = ((int)blockIdx.x - point_blocks) * 256 + threadIdx.x;
    if (i >= n_lines) return;
    float out4[4];
    associate_line(P, depth, lines + 8 * (size_t)i, out4);
    for (int k = 0; k < 4; ++k) line_out[4 * (size_t)i + k] = out4[k];
  }
}

int check_image(const float* depth, int width, int height, int depth_pitch) {
  PLVS_REQUIRE(depth, "null depth image");
  PLVS_REQUIRE(width > 0 && height > 0 && depth_pitch >= width, "bad depth image size (depth_pitch is in floats, >= width)");
  return PLVS_OK;
}

// Both loops, one launch.  h_depth != NULL: the image is uploaded behind the arrays (the host flavours); otherwise d_depth
// is read where it lies.  K4 may be NULL when there are no lines.  The outputs are host arrays: the call ends with a wait.
int associate(const plvs_keypoint* kps, const plvs_keypoint* kps_un, int n, const plvs_keyline* kl, const plvs_keyline* klu, int nl,
              const float* h_depth, const float* d_depth, int width, int height, int pitch, const float* K4, float mbf,
              float min_line_length_3d, float* u_right, float* depth_out, float* u_right_start, float* depth_start,
              float* u_right_end, float* depth_end, hipStream_t stream, bool own_stream) {
  if (n == 0 && nl == 0) return PLVS_OK;
  RgbdParams P;
  P.width = width; P.height = height; P.pitch = pitch;
  P.cx = P.cy = P.invfx = P.invfy = 0.0f;
  if (nl > 0) {
    P.cx = K4[2]; P.cy = K4[3];
    P.invfx = 1.0f / K4[0]; P.invfy = 1.0f / K4[1];
  }
  P.mbf = mbf;
  P.min_line_length_3d = min_line_length_3d;
  P.cos_view_z_angle_max = plvs::cos_view_z_angle_max();   // kCosViewZAngleMax (:103)
  plvs::HostStage& st = plvs::thread_stage();
  const size_t f_in = 3 * (size_t)n + 8 * (size_t)nl, f_out = 2 * (size_t)n + 4 * (size_t)nl;
  const size_t o_out = (sizeof(float) * f_in + 15) & ~(size_t)15, o_img = o_out + ((sizeof(float) * f_out + 15) & ~(size_t)15);
  const size_t b_img = h_depth ? sizeof(float) * ((size_t)pitch * (size_t)(height - 1) + (size_t)width) : 0;   // (the last row ends at its width)
  PLVS_HIP_TRY(st.reserve(o_img + b_img + 16));
  if (own_stream) stream = st.stream;
  float* in = reinterpret_cast<float*>(st.pinned);
  for (int i = 0; i < n; ++i) {
    in[3 * i] = kps[i].x;
    in[3 * i + 1] = kps[i].y;
    in[3 * i + 2] = kps_un[i].x;
  }
  float* lin = in + 3 * (size_t)n;
  for (int i = 0; i < nl; ++i) {
    lin[8 * i] = kl[i].startPointX; lin[8 * i + 1] = kl[i].startPointY;
    lin[8 * i + 2] = kl[i].endPointX; lin[8 * i + 3] = kl[i].endPointY;
    lin[8 * i + 4] = klu[i].startPointX; lin[8 * i + 5] = klu[i].startPointY;
    lin[8 * i + 6] = klu[i].endPointX; lin[8 * i + 7] = klu[i].endPointY;
  }
  PLVS_HIP_TRY(hipMemcpyAsync(st.dev, st.pinned, sizeof(float) * f_in, hipMemcpyHostToDevice, stream));
  if (h_depth) {
    memcpy(st.pinned + o_img, h_depth, b_img);
    PLVS_HIP_TRY(hipMemcpyAsync(st.dev + o_img, st.pinned + o_img, b_img, hipMemcpyHostToDevice, stream));
    d_depth = reinterpret_cast<const float*>(st.dev + o_img);
  }
  const int point_blocks = (int)plvs::ceil_div((size_t)n, 256), line_blocks = (int)plvs::ceil_div((size_t)nl, 256);
  const float* d_in = reinterpret_cast<const float*>(st.dev);
  float* d_out = reinterpret_cast<float*>(st.dev + o_out);
  hipLaunchKernelGGL(rgbd_associate_kernel, dim3(point_blocks + line_blocks), dim3(256), 0, stream, P, d_depth, d_in, n, point_blocks,
                     d_in + 3 * (size_t)n, nl, d_out, d_out + 2 * (size_t)n);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(hipMemcpyAsync(st.pinned + o_out, st.dev + o_out, sizeof(float) * f_out, hipMemcpyDeviceToHost, stream));
  PLVS_HIP_TRY(hipStreamSynchronize(stream));
  const float* out = reinterpret_cast<const float*>(st.pinned + o_out);
  for (int i = 0; i < n; ++i) {
    u_right[i] = out[2 * i];
    depth_out[i] = out[2 * i + 1];
  }
  const float* lout = out + 2 * (size_t)n;
  for (int i = 0; i < nl; ++i) {
    u_right_start[i] = lout[4 * i];
    depth_start[i] = lout[4 * i + 1];
    u_right_end[i] = lout[4 * i + 2];
    depth_end[i] = lout[4 * i + 3];
  }
  return PLVS_OK;
}

}  // namespace

extern "C" {

int plvs_hip_frame_compute_stereo_from_rgbd(const plvs_keypoint* kps, const plvs_keypoint* kps_un, int n, const float* depth, int width,
                                            int height, int depth_pitch, float mbf, float* u_right, float* depth_out) {
  PLVS_REQUIRE(n >= 0 && (n == 0 || (kps && kps_un && u_right && depth_out)), "bad arguments");
  const int rc = check_image(depth, width, height, depth_pitch);
  if (rc != PLVS_OK) return rc;
  return associate(kps, kps_un, n, nullptr, nullptr, 0, depth, nullptr, width, height, depth_pitch, nullptr, mbf, 0.0f, u_right,
                   depth_out, nullptr, nullptr, nullptr, nullptr, nullptr, true);
}

int plvs_hip_frame_compute_stereo_lines_from_rgbd(const plvs_keyline* keylines, const plvs_keyline* keylines_un, int n, const float* depth,
                                                  int width, int height, int depth_pitch, const float* K4, float mbf,
                                                  float min_line_length_3d, float* u_right_start, float* depth_start,
                                                  float* u_right_end, float* depth_end) {
  PLVS_REQUIRE(n >= 0 && K4 && (n == 0 || (keylines && keylines_un && u_right_start && depth_start && u_right_end && depth_end)),
               "bad arguments");
  const int rc = check_image(depth, width, height, depth_pitch);
  if (rc != PLVS_OK) return rc;
  return associate(nullptr, nullptr, 0, keylines, keylines_un, n, depth, nullptr, width, height, depth_pitch, K4, mbf,
                   min_line_length_3d, nullptr, nullptr, u_right_start, depth_start, u_right_end, depth_end, nullptr, true);
}

int plvs_hip_frame_stereo_from_rgbd_dev(const plvs_keypoint* kps, const plvs_keypoint* kps_un, int n, const plvs_keyline* keylines,
                                        const plvs_keyline* keylines_un, int n_lines, const float* d_depth, int width, int height,
                                        int depth_pitch, const float* K4, float mbf, float min_line_length_3d, float* u_right,
                                        float* depth_out, float* u_right_start, float* depth_start, float* u_right_end,
                                        float* depth_end, void* stream) {
  PLVS_REQUIRE(n >= 0 && (n == 0 || (kps && kps_un && u_right && depth_out)), "bad key point arguments");
  PLVS_REQUIRE(n_lines >= 0 &&
                   (n_lines == 0 || (K4 && keylines && keylines_un && u_right_start && depth_start && u_right_end && depth_end)),
               "bad line arguments");
  const int rc = check_image(d_depth, width, height, depth_pitch);
  if (rc != PLVS_OK) return rc;
  return associate(kps, kps_un, n, keylines, keylines_un, n_lines, nullptr, d_depth, width, height, depth_pitch, K4, mbf,
                   min_line_length_3d, u_right, depth_out, u_right_start, depth_start, u_right_end, depth_end,
                   static_cast<hipStream_t>(stream), false);
}

int plvs_hip_frame_scene_median_depth(const float* depth, int n, float fallback, float* median) {
  PLVS_REQUIRE(median && n >= 0 && (n == 0 || depth), "bad arguments");
  std::vector<float> v;
  v.reserve((size_t)n);
  for (int i = 0; i < n; ++i)
    if (depth[i] > 0) v.push_back(depth[i]);
  float res = fallback;
  if (!v.empty()) {
    std::sort(v.begin(), v.end());
    res = v[(v.size() - 1) / 2];
  }
  *median = res;
  return PLVS_OK;
}

int plvs_hip_frame_rgbd_dev(plvs_orb* orb, plvs_lines* lines, const uint8_t* d_image, int w, int hh, int stride, const float* d_depth,
                            int depth_pitch, const plvs_rgbd_calib* calib, plvs_rgbd_frame* f, void* stream) {
  PLVS_REQUIRE(orb && d_image && calib && f, "null argument");
  PLVS_REQUIRE(w > 0 && hh > 0 && stride >= w, "bad image size");
  const int rc_img = check_image(d_depth, w, hh, depth_pitch);
  if (rc_img != PLVS_OK) return rc_img;
  PLVS_REQUIRE(f->kp_cap > 0 && f->kps && f->kps_un && f->desc && f->u_right && f->depth && f->cell_start && f->cell_items,
               "key point outputs / capacity");
  PLVS_REQUIRE(!lines || (f->line_cap > 0 && f->keylines && f->keylines_un && f->line_desc && f->u_right_start && f->depth_start &&
                          f->u_right_end && f->depth_end),
               "line outputs / capacity");
  PLVS_REQUIRE(calib->ndist == 0 || calib->ndist == 4 || calib->ndist == 5 || calib->ndist == 8, "4, 5 or 8 distortion coefficients");
  f->n_kp = f->n_lines = f->n_items = 0;
  f->mono_index = -1;
  f->median_depth = calib->median_fallback;
  // 1. ExtractORB / ExtractLSD (:498-517), lapping (0, 0)
  int n = 0, mono = -1, nl = 0;
  const int rc = lines ? plvs_hip_frame_extract_dev(orb, lines, d_image, w, hh, stride, 0, 0, f->kps, f->desc, f->kp_cap, &n, &mono,
                                                    f->keylines, f->line_desc, f->line_cap, &nl)
                       : plvs_hip_orb_extract_dev(orb, d_image, w, hh, stride, 0, 0, f->kps, f->desc, f->kp_cap, &n, &mono);
  if (rc != PLVS_OK) return rc;
  if (n > f->kp_cap || nl > f->line_cap) {
    plvs::set_error("frame: %d key points / %d lines exceed the capacities %d / %d", n, nl, f->kp_cap, lines ? f->line_cap : 0);
    return PLVS_ERR_CAPACITY;
  }
  f->mono_index = mono;
  if (n == 0) {   // if(mvKeys.empty()) return;  (:544-545 — before the lines are touched)
    for (int c = 0; c <= kGridCells; ++c) f->cell_start[c] = 0;
    return PLVS_OK;
  }
  // 2. UndistortKeyPoints (:547)
  int rc2 = plvs_hip_frame_undistort_keypoints(f->kps, n, calib->K4, calib->dist, calib->ndist, f->kps_un);
  if (rc2 != PLVS_OK) return rc2;
  // 4a. UndistortKeyLines (:569) and the compaction of mvKeyLines / mLineDescriptors it does (:1649-1655) — ahead of the
  // point association, which does not depend on it, so that both associations share the launch
  if (nl > 0) {
    std::vector<int32_t> kept((size_t)nl);
    int m = 0;
    rc2 = plvs_hip_frame_undistort_keylines(f->keylines, nl, calib->K4, calib->dist, calib->ndist, calib->bounds4, f->keylines_un,
                                            kept.data(), &m);
    if (rc2 != PLVS_OK) return rc2;
    for (int j = 0; j < m; ++j)   // kept ascends: in place
      if (kept[j] != j) {
        f->keylines[j] = f->keylines[kept[j]];
        memcpy(f->line_desc + 32 * (size_t)j, f->line_desc + 32 * (size_t)kept[j], 32);
      }
    nl = m;
  }
  // 3. + 4b. ComputeStereoFromRGBD (:549), ComputeStereoLinesFromRGBD (:572)
  rc2 = associate(f->kps, f->kps_un, n, f->keylines, f->keylines_un, nl, nullptr, d_depth, w, hh, depth_pitch, calib->K4, calib->mbf,
                  calib->min_line_length_3d, f->u_right, f->depth, f->u_right_start, f->depth_start, f->u_right_end, f->depth_end,
                  static_cast<hipStream_t>(stream), false);
  if (rc2 != PLVS_OK) return rc2;
  if (calib->use_median_depth) {
    rc2 = plvs_hip_frame_scene_median_depth(f->depth, n, calib->median_fallback, &f->median_depth);
    if (rc2 != PLVS_OK) return rc2;
  }
  // 5. AssignFeaturesToGrid
  int items = 0;
  rc2 = plvs_hip_frame_assign_features_to_grid(f->kps_un, n, calib->bounds4[0], calib->bounds4[2], calib->grid_w_inv, calib->grid_h_inv,
                                               f->cell_start, f->cell_items, &items);
  if (rc2 != PLVS_OK) return rc2;
  f->n_kp = n;
  f->n_lines = nl;
  f->n_items = items;
  return PLVS_OK;
}

}  // extern "C"
