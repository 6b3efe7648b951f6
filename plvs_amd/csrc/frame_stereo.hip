// What makes a frame stereo on the line side: Frame::ComputeStereoLineMatches (reference src/Frame.cc:2008-2248) with
// LineMatcher::SearchStereoMatchesByKnn (src/LineMatcher.cc:454-586) and ComputeDescriptorMatches (:2568-2620) inside it,
// as ONE launch of ONE workgroup — and the stereo constructor (src/Frame.cc:214-398) as one call over the entries of
// frame.hip / frame_glue.hip / stereo.hip.
//
// The workgroup: 1024 threads = 16 waves; both sides' descriptors and the six key-line fields the function reads sit in LDS
// (56 KB at the capacity of 512 lines per side).  Stages, a barrier between each two:
//   1. exact k = 2 search, left = query, right = train, a wave per query striding over the queries, the multi-index-hash
//      tie order (hamming_key.hpp, the key of hamming_knn2_kernel<true>).  Lane 0 applies the query's tests — ratio test
//      when a second neighbour exists, d0 < descriptor_dist, equal octaves — and a passing query q names right line t:
//        holder[t] = min (d0 << 16 | q)     first[t] = min q
//      "Replace with better" (:490-540) without order: the holder is the passing query with the smallest distance, among
//      equal distances the lowest index (the replacement at :517 is strict); vMatches lists the right lines by the lowest
//      passing query that named them.  run_pass of line_search.hip is the host statement of the same rule.
//   2. thread t < 512 = right line t.  The holders' rotation bins go into the 12-bin histogram; ComputeThreeMaxima (every thread
//      reads the 12 counts) cuts the others.
//   3. the per-match geometry of :2058-2220, a lane per match: the matches are independent.  vFlagMatchedRight (:2068) can
//      never reject — every right line occurs once in vMatches — and the +-1 octave test (:2078) can never reject after the
//      equal-octave test of the matcher; neither is restated.  Survivors count their integer distance into 257 bins.
//   4. the median cut (:2224-2243): the sorted pairs (int(distance), idxL) have `first` of element size / 2 as median — a
//      prefix sum over the bins finds it, no sort; survivors with first >= 1.5f * 1.48f * median (int against float) are
//      reset.  The order of vMatches never reaches an output: every stage above is a function of sets.
//
// Arithmetic: the reference's own sequence (frame_geom.hpp), f32 where it computes in float, f64 where it builds
// Eigen::Vector3d; -ffp-contract=off, correctly rounded `/` and sqrt.  tests/golden/frame_stereo_reference.npz — the
// reference's run — decides every evaluation order; every output float equals it bit for bit.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <thread>

#include "common.hpp"
#include "frame_geom.hpp"
#include "hamming_key.hpp"
#include "stereo_internal.hpp"

namespace {

using plvs::V3;

constexpr int kLineCap = 512;          // lines per side
constexpr int kThreads = 1024;         // 16 waves share the queries of stage 1; from stage 2 on thread t < kLineCap = right line t
constexpr int kHistoLength = 12;       // LineMatcher::HISTO_LENGTH, src/LineMatcher.cc:90
constexpr int kDistBins = 257;         // Hamming distances of 256-bit descriptors: 0..256
constexpr int kLineWords = 6;          // angle, octave, startPointX, startPointY, endPointX, endPointY
constexpr int kGridCells = 64 * 48;    // FRAME_GRID_COLS x FRAME_GRID_ROWS, include/Frame.h:67-68
constexpr unsigned kNone = ~0u;

struct StereoLineParams {
  int n, n_right;
  float cx, cy, invfx, invfy, mbf;
  float min_d, max_d;                  // the disparity window (:2023-2026), float
  float min_line_length_3d;            // Frame::skMinLineLength3D
  float cos_view_z_angle_max;          // Frame::kCosViewZAngleMax, computed on the host
  float nn_ratio;                      // LineMatcher::mfNNratio
  int check_orientation;               // LineMatcher::mbCheckOrientation
  int descriptor_dist;                 // LineMatcher::TH_LOW_STEREO
};

// Geom2DUtils::areLinesEqual (include/Geom2DUtils.h:162-180): float on values narrowed from double, one fabs(1. - ...) in double
__device__ __forceinline__ bool lines_equal(const V3& l1, const V3& l2, float dot_threshold, float dist_threshold) {
  const float normals_dot = (float)(l1.x * l2.x + l1.y * l2.y);
  float d1 = (float)l1.z;
  const float d2 = (float)l2.z;
  if (fabs(1. - (double)fabsf(normals_dot)) < (double)dot_threshold) {
    if (normals_dot < 0) d1 *= -1;
    if (fabsf(d1 - d2) < dist_threshold) return true;
  }
  return false;
}

// lineSegmentOverlapStereo (src/Frame.cc:1986-2005)
__device__ __forceinline__ double overlap_stereo(double ys1, double ye1, double ys2, double ye2) {
  const double ymin1 = ys1 < ye1 ? ys1 : ye1, ymax1 = ys1 < ye1 ? ye1 : ys1;
  const double ymin2 = ys2 < ye2 ? ys2 : ye2, ymax2 = ys2 < ye2 ? ye2 : ys2;
  if (ymax2 < ymin1 || ymin2 > ymax1) return 0.;
  return (ymax1 < ymax2 ? ymax1 : ymax2) - (ymin1 > ymin2 ? ymin1 : ymin2);
}

// One match of :2070-2219.  l, r: startPointX, startPointY, endPointX, endPointY of the left / right line; sigma2 =
// mvLineLevelSigma2[left octave].  false: the left line stays mono.
__device__ __forceinline__ bool triangulate(const StereoLineParams& P, float sigma2, const float* l, const float* r, float* out4) {
  const float sigma = sqrtf(sigma2);
  const float uS = l[0], vS = l[1], uE = l[2], vE = l[3];
  const float dyl = fabsf(l[1] - l[3]), dyr = fabsf(r[1] - r[3]);
  const float min_span = 2.0f * sigma;                                         // kMinVerticalLineSpan
  if (dyl <= min_span || dyr <= min_span) return false;
  const double overlap = overlap_stereo(l[1], l[3], r[1], r[3]);
  if (overlap <= (double)(2.0f * sigma)) return false;                         // kMinStereoLineOverlap
  const V3 startL = plvs::v3(l[0], l[1], 1.0f), endL = plvs::v3(l[2], l[3], 1.0f);
  V3 ll = plvs::cross(startL, endL);
  ll = plvs::divided(ll, sqrt(ll.x * ll.x + ll.y * ll.y));
  const V3 startR = plvs::v3(r[0], r[1], 1.0f), endR = plvs::v3(r[2], r[3], 1.0f);
  V3 lr = plvs::cross(startR, endR);
  lr = plvs::divided(lr, sqrt(lr.x * lr.x + lr.y * lr.y));
  const float dot_threshold = 0.005f * sigma;                                  // kLineNormalsDotProdThreshold
  const float dist_threshold = 2.f * sigma;
  if (fabs(ll.x) < (double)dot_threshold) return false;
  if (fabs(lr.x) < (double)dot_threshold) return false;
  if (lines_equal(ll, lr, dot_threshold, dist_threshold)) return false;
  const double disparity_s = plvs::dot(lr, startL) / lr.x;
  const double disparity_e = plvs::dot(lr, endL) / lr.x;
  const double min_d = (double)P.min_d, max_d = (double)P.max_d;
  if (!(disparity_s >= min_d && disparity_s <= max_d && disparity_e >= min_d && disparity_e <= max_d)) return false;
  float dS = (float)((double)P.mbf / disparity_s), dE = (float)((double)P.mbf / disparity_e);
  out4[0] = (float)(startL.x - disparity_s);
  out4[1] = dS;
  out4[2] = (float)(endL.x - disparity_e);
  out4[3] = dE;
  if (dS > 0 && dE > 0) {
    const float xS = (uS - P.cx) * dS * P.invfx, yS = (vS - P.cy) * dS * P.invfy;
    const float xE = (uE - P.cx) * dE * P.invfx, yE = (vE - P.cy) * dE * P.invfy;
    const V3 camRay = plvs::normalized(plvs::v3(xS, yS, dS));
    const V3 lineES = plvs::v3(xS - xE, yS - yE, dS - dE);
    const double length = plvs::norm(lineES);
    if (length < (double)P.min_line_length_3d) {
      dS = dE = -1;
    } else {
      const float cos_view_angle = fabsf((float)plvs::dot(camRay, plvs::divided(lineES, length)));
      if (cos_view_angle > P.cos_view_z_angle_max) dS = dE = -1;
    }
  }
  return dS > 0 && dE > 0;
}

// lines: kLineWords per line.  out: 4 floats per left line (uRightStart, depthStart, uRightEnd, depthEnd), then one int:
// the lines left with depth.  holders (nullable, a debug output of stage 1 / 2): per right line its holder (-1 none), the
// distance, valid after the rotation check, and the lowest query that named it.
__global__ __launch_bounds__(kThreads) void stereo_line_matches_kernel(StereoLineParams P, const uint4* __restrict__ desc_l,
                                                                       const uint4* __restrict__ desc_r,
                                                                       const uint32_t* __restrict__ lines_l,
                                                                       const uint32_t* __restrict__ lines_r,
                                                                       const float* __restrict__ sigma2, float* __restrict__ out,
                                                                       int32_t* __restrict__ holders) {
  __shared__ uint4 s_dl[2 * kLineCap], s_dr[2 * kLineCap];
  __shared__ uint32_t s_ll[kLineWords * kLineCap], s_lr[kLineWords * kLineCap];
  __shared__ unsigned s_holder[kLineCap], s_first[kLineCap];
  __shared__ int s_hist[kHistoLength], s_bins[kDistBins], s_median, s_stereo;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = P.n, nr = P.n_right;   // 1..kLineCap: the host has checked
  for (int i = tid; i < 2 * n; i += kThreads) s_dl[i] = desc_l[i];
  for (int i = tid; i < 2 * nr; i += kThreads) s_dr[i] = desc_r[i];
  for (int i = tid; i < kLineWords * n; i += kThreads) s_ll[i] = lines_l[i];
  for (int i = tid; i < kLineWords * nr; i += kThreads) s_lr[i] = lines_r[i];
  for (int i = tid; i < 4 * n; i += kThreads) out[i] = -1.0f;
  if (tid < kLineCap) s_holder[tid] = s_first[tid] = kNone;
  if (tid < kHistoLength) s_hist[tid] = 0;
  if (tid < kDistBins) s_bins[tid] = 0;
  if (tid == 0) s_median = s_stereo = 0;
  __syncthreads();

  // 1. the k = 2 search and the tests of one query
  for (int q = wave; q < n; q += kThreads / 64) {
    const uint4 qa = s_dl[2 * q], qb = s_dl[2 * q + 1];
    const uint32_t qw[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
    unsigned long long b1 = plvs::kNoKey, b2 = plvs::kNoKey;
    for (int t = lane; t < nr; t += 64) {
      const uint4 ta = s_dr[2 * t], tb = s_dr[2 * t + 1];
      const uint32_t x[8] = {ta.x ^ qw[0], ta.y ^ qw[1], ta.z ^ qw[2], ta.w ^ qw[3], tb.x ^ qw[4], tb.y ^ qw[5], tb.z ^ qw[6], tb.w ^ qw[7]};
      plvs::insert_key(plvs::hamming_key<true>(x, t), b1, b2);
    }
    plvs::merge_keys_wave(b1, b2);
    if (lane == 0) {   // (nr >= 1: a first neighbour exists)
      const int t = plvs::key_index(b1);
      const float d0 = (float)plvs::key_distance(b1);
      bool pass = b2 == plvs::kNoKey || d0 < P.nn_ratio * (float)plvs::key_distance(b2);    // ComputeDescriptorMatches :2606-2618
      pass = pass && d0 < (float)P.descriptor_dist;                                          // :485
      pass = pass && s_ll[kLineWords * q + 1] == s_lr[kLineWords * t + 1];                   // :487 octaves
      if (pass) {
        atomicMin(&s_holder[t], ((unsigned)plvs::key_distance(b1) << 16) | (unsigned)q);
        atomicMin(&s_first[t], (unsigned)q);
      }
    }
  }
  __syncthreads();

  // 2. thread t = right line t: the rotation histogram over the holders
  const int t = tid;
  const unsigned hold = t < kLineCap ? s_holder[t] : kNone;   // (kNone beyond nr: nobody named it)
  const bool held = hold != kNone;
  const int q = held ? (int)(hold & 0xffffu) : -1, dist = held ? (int)(hold >> 16) : 0;
  int bin = -1;
  if (held && P.check_orientation) {
    const float two_pi = (float)(2.0 * M_PI);              // M_2PI, src/LineMatcher.cc:57
    const float factor = kHistoLength / two_pi;            // :470
    float rot = __uint_as_float(s_ll[kLineWords * q]) - __uint_as_float(s_lr[kLineWords * t]);
    if (rot < 0.0) rot += two_pi; else if (rot > two_pi) rot -= two_pi;
    bin = (int)roundf(rot * factor);
    if (bin == kHistoLength) bin = 0;
    bin = bin < 0 ? 0 : (bin >= kHistoLength ? kHistoLength - 1 : bin);   // (the reference asserts the range; angles are in [-pi, pi])
    atomicAdd(&s_hist[bin], 1);
  }
  __syncthreads();
  bool valid = held;
  if (P.check_orientation) {
    int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < kHistoLength; ++i) {     // ComputeThreeMaxima, :101-143
      const int s = s_hist[i];
      if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
      else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
      else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
    valid = held && (bin == ind1 || bin == ind2 || bin == ind3);
  }
  if (holders != nullptr && t < nr) {
    holders[4 * t] = q;
    holders[4 * t + 1] = dist;
    holders[4 * t + 2] = valid ? 1 : 0;
    holders[4 * t + 3] = held ? (int)s_first[t] : -1;
  }

  // 3. the geometry of the match (q, t)
  float out4[4];
  bool survives = false;
  if (valid) {
    float l[4], r[4];
    for (int k = 0; k < 4; ++k) {
      l[k] = __uint_as_float(s_ll[kLineWords * q + 2 + k]);
      r[k] = __uint_as_float(s_lr[kLineWords * t + 2 + k]);
    }
    survives = triangulate(P, sigma2[(int)s_ll[kLineWords * q + 1]], l, r, out4);   // (octaves inside the table: the host has checked)
    if (survives) atomicAdd(&s_bins[dist], 1);
  }
  __syncthreads();

  // 4. the median of the survivors' distances: lane l of wave 0 owns bins 5 l .. 5 l + 4
  if (wave == 0) {
    int c[5], own = 0;
    for (int j = 0; j < 5; ++j) {
      const int b = 5 * lane + j;
      c[j] = b < kDistBins ? s_bins[b] : 0;
      own += c[j];
    }
    int incl = own;
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    const int total = __shfl(incl, 63, 64), k = total / 2;   // vDistIdx[vDistIdx.size() / 2]
    int run = incl - own;
    if (total > 0 && run <= k && k < incl)
      for (int j = 0; j < 5; ++j) {
        run += c[j];
        if (k < run) {
          s_median = 5 * lane + j;
          break;
        }
      }
  }
  __syncthreads();
  if (survives) {
    const float median = (float)s_median;
    const float th_dist = 1.5f * 1.48f * median;
    if ((float)dist < th_dist) {   // :2233, int against float
      for (int k = 0; k < 4; ++k) out[4 * q + k] = out4[k];
      atomicAdd(&s_stereo, 1);
    }
  }
  __syncthreads();
  if (tid == 0) reinterpret_cast<int*>(out)[4 * n] = s_stereo;
}

int check_line_args(const plvs_keyline* klu, const uint8_t* desc, int n, const plvs_keyline* klr, const uint8_t* desc_r, int n_right,
                    const float* sigma2, int n_levels, const float* K4, float* u_right_start, float* depth_start, float* u_right_end,
                    float* depth_end) {
  PLVS_REQUIRE(n >= 0 && n_right >= 0, "negative count");
  PLVS_REQUIRE(n == 0 || (klu && desc && u_right_start && depth_start && u_right_end && depth_end), "null left array or output");
  PLVS_REQUIRE(n_right == 0 || (klr && desc_r), "null right array");
  if (n == 0 || n_right == 0) return PLVS_OK;
  PLVS_REQUIRE(sigma2 && n_levels > 0 && K4, "null level table or calibration");
  if (n > kLineCap || n_right > kLineCap) {
    plvs::set_error("stereo line matches: %d / %d lines exceed the capacity of %d per side", n, n_right, kLineCap);
    return PLVS_ERR_CAPACITY;
  }
  for (int i = 0; i < n; ++i) PLVS_REQUIRE(klu[i].octave >= 0 && klu[i].octave < n_levels, "left octave outside the level table");
  for (int i = 0; i < n_right; ++i) PLVS_REQUIRE(klr[i].octave >= 0 && klr[i].octave < n_levels, "right octave outside the level table");
  return PLVS_OK;
}

void pack_lines(const plvs_keyline* kl, int n, uint32_t* dst) {
  for (int i = 0; i < n; ++i) {
    const float f[kLineWords] = {kl[i].angle, 0.0f, kl[i].startPointX, kl[i].startPointY, kl[i].endPointX, kl[i].endPointY};
    memcpy(dst + kLineWords * (size_t)i, f, sizeof f);
    dst[kLineWords * (size_t)i + 1] = (uint32_t)kl[i].octave;
  }
}

// Arguments checked by check_line_args.  holders: host, 4 x n_right ints, or NULL.
int line_matches(const plvs_keyline* klu, const uint8_t* desc, int n, const plvs_keyline* klr, const uint8_t* desc_r, int n_right,
                 const float* sigma2, int n_levels, const float* K4, float mbf, float line_stereo_max_dist, float min_line_length_3d,
                 float nn_ratio, int check_orientation, int descriptor_dist, float* u_right_start, float* depth_start,
                 float* u_right_end, float* depth_end, int* n_stereo, int32_t* holders, hipStream_t stream) {
  if (n_stereo) *n_stereo = 0;
  if (n == 0 || n_right == 0) {   // :2037-2045: all -1, nothing launched
    for (int i = 0; i < n; ++i) u_right_start[i] = depth_start[i] = u_right_end[i] = depth_end[i] = -1.0f;
    return PLVS_OK;
  }
  StereoLineParams P;
  P.n = n; P.n_right = n_right;
  P.cx = K4[2]; P.cy = K4[3];
  P.invfx = 1.0f / K4[0]; P.invfy = 1.0f / K4[1];
  P.mbf = mbf;
  const float mb = mbf / K4[0];                                     // Frame::mb (:390)
  const float min_z = mb, max_z = std::min(mbf, line_stereo_max_dist);   // :2023-2024
  P.min_d = mbf / max_z;
  P.max_d = mbf / min_z;
  P.min_line_length_3d = min_line_length_3d;
  P.cos_view_z_angle_max = plvs::cos_view_z_angle_max();
  P.nn_ratio = nn_ratio;
  P.check_orientation = check_orientation;
  P.descriptor_dist = descriptor_dist;
  using plvs::up16;
  const size_t o_dl = 0, o_dr = o_dl + up16(32 * (size_t)n), o_ll = o_dr + up16(32 * (size_t)n_right),
               o_lr = o_ll + up16(4 * kLineWords * (size_t)n), o_s2 = o_lr + up16(4 * kLineWords * (size_t)n_right),
               o_out = o_s2 + up16(4 * (size_t)n_levels), b_out = up16(4 * (4 * (size_t)n + 1)), o_hold = o_out + b_out,
               b_hold = holders ? up16(16 * (size_t)n_right) : 0;
  plvs::HostStage& st = plvs::thread_stage();
  PLVS_HIP_TRY(st.reserve(o_hold + b_hold));
  memcpy(st.pinned + o_dl, desc, 32 * (size_t)n);
  memcpy(st.pinned + o_dr, desc_r, 32 * (size_t)n_right);
  pack_lines(klu, n, reinterpret_cast<uint32_t*>(st.pinned + o_ll));
  pack_lines(klr, n_right, reinterpret_cast<uint32_t*>(st.pinned + o_lr));
  memcpy(st.pinned + o_s2, sigma2, 4 * (size_t)n_levels);
  PLVS_HIP_TRY(hipMemcpyAsync(st.dev, st.pinned, o_out, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(stereo_line_matches_kernel, dim3(1), dim3(kThreads), 0, stream, P, reinterpret_cast<const uint4*>(st.dev + o_dl),
                     reinterpret_cast<const uint4*>(st.dev + o_dr), reinterpret_cast<const uint32_t*>(st.dev + o_ll),
                     reinterpret_cast<const uint32_t*>(st.dev + o_lr), reinterpret_cast<const float*>(st.dev + o_s2),
                     reinterpret_cast<float*>(st.dev + o_out), holders ? reinterpret_cast<int32_t*>(st.dev + o_hold) : nullptr);
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(hipMemcpyAsync(st.pinned + o_out, st.dev + o_out, b_out + b_hold, hipMemcpyDeviceToHost, stream));
  PLVS_HIP_TRY(hipStreamSynchronize(stream));
  const float* out = reinterpret_cast<const float*>(st.pinned + o_out);
  for (int i = 0; i < n; ++i) {
    u_right_start[i] = out[4 * i];
    depth_start[i] = out[4 * i + 1];
    u_right_end[i] = out[4 * i + 2];
    depth_end[i] = out[4 * i + 3];
  }
  if (n_stereo) memcpy(n_stereo, out + 4 * (size_t)n, sizeof(int));
  if (holders) memcpy(holders, st.pinned + o_hold, 16 * (size_t)n_right);
  return PLVS_OK;
}

}  // namespace

extern "C" {

int plvs_hip_frame_compute_stereo_line_matches(const plvs_keyline* keylines_un, const uint8_t* desc, int n,
                                               const plvs_keyline* keylines_right_un, const uint8_t* desc_right, int n_right,
                                               const float* line_level_sigma2, int n_levels, const float* K4, float mbf,
                                               float line_stereo_max_dist, float min_line_length_3d, float nn_ratio,
                                               int check_orientation, int descriptor_dist, float* u_right_start, float* depth_start,
                                               float* u_right_end, float* depth_end, int* n_stereo, void* stream) {
  const int rc = check_line_args(keylines_un, desc, n, keylines_right_un, desc_right, n_right, line_level_sigma2, n_levels, K4,
                                 u_right_start, depth_start, u_right_end, depth_end);
  if (rc != PLVS_OK) return rc;
  return line_matches(keylines_un, desc, n, keylines_right_un, desc_right, n_right, line_level_sigma2, n_levels, K4, mbf,
                      line_stereo_max_dist, min_line_length_3d, nn_ratio, check_orientation, descriptor_dist, u_right_start,
                      depth_start, u_right_end, depth_end, n_stereo, nullptr, static_cast<hipStream_t>(stream));
}

// The same with the matcher stage's result per right line (holder, distance, valid, first naming query): what the tests
// hold against plvs_hip_lines_search_stereo_by_knn.
int plvs_hip_frame_compute_stereo_line_matches_debug(const plvs_keyline* keylines_un, const uint8_t* desc, int n,
                                                     const plvs_keyline* keylines_right_un, const uint8_t* desc_right, int n_right,
                                                     const float* line_level_sigma2, int n_levels, const float* K4, float mbf,
                                                     float line_stereo_max_dist, float min_line_length_3d, float nn_ratio,
                                                     int check_orientation, int descriptor_dist, float* u_right_start,
                                                     float* depth_start, float* u_right_end, float* depth_end, int* n_stereo,
                                                     int32_t* holders4, void* stream) {
  PLVS_REQUIRE(holders4 || n_right == 0, "null holders");
  const int rc = check_line_args(keylines_un, desc, n, keylines_right_un, desc_right, n_right, line_level_sigma2, n_levels, K4,
                                 u_right_start, depth_start, u_right_end, depth_end);
  if (rc != PLVS_OK) return rc;
  return line_matches(keylines_un, desc, n, keylines_right_un, desc_right, n_right, line_level_sigma2, n_levels, K4, mbf,
                      line_stereo_max_dist, min_line_length_3d, nn_ratio, check_orientation, descriptor_dist, u_right_start,
                      depth_start, u_right_end, depth_end, n_stereo, n && n_right ? holders4 : nullptr,
                      static_cast<hipStream_t>(stream));
}

int plvs_hip_frame_stereo_dev(plvs_orb* orb_left, plvs_orb* orb_right, plvs_lines* lines_left, plvs_lines* lines_right,
                              plvs_stereo* stereo, const uint8_t* d_left, const uint8_t* d_right, int w, int hh, int stride,
                              const plvs_stereo_calib* calib, plvs_stereo_frame* f, void* stream) {
  PLVS_REQUIRE(orb_left && orb_right && stereo && d_left && d_right && calib && f, "null argument");
  PLVS_REQUIRE((lines_left == nullptr) == (lines_right == nullptr), "both line extractors or neither");
  PLVS_REQUIRE(w > 0 && hh > 0 && stride >= w, "bad image size");
  PLVS_REQUIRE(plvs::stereo_made_from(stereo, orb_left, orb_right), "the plvs_stereo was not created from these two ORB extractors");
  PLVS_REQUIRE(calib->ndist >= 0 && calib->ndist <= 8 && (calib->ndist == 0 || calib->dist[0] == 0.0f),
               "the stereo constructor takes a rectified pair (no distortion)");
  PLVS_REQUIRE(f->kp_cap > 0 && f->kps && f->kps_un && f->desc && f->u_right && f->depth && f->cell_start && f->cell_items,
               "left key point outputs / capacity");
  PLVS_REQUIRE(f->kp_right_cap > 0 && f->kps_right && f->desc_right, "right key point outputs / capacity");
  const bool with_lines = lines_left != nullptr;
  PLVS_REQUIRE(!with_lines || (f->line_cap > 0 && f->keylines && f->keylines_un && f->line_desc && f->u_right_start && f->depth_start &&
                               f->u_right_end && f->depth_end && f->line_right_cap > 0 && f->keylines_right && f->keylines_right_un &&
                               f->line_desc_right && calib->line_level_sigma2 && calib->n_line_levels > 0),
               "line outputs / capacities / level table");
  f->n_kp = f->n_kp_right = f->n_lines = f->n_lines_right = f->n_items = f->n_stereo_points = f->n_stereo_lines = 0;
  f->mono_index = f->mono_index_right = -1;
  // 1. the four extractions (:314-323; two without line extractors, :328-331), lapping (0, 0): the right image on a thread
  // of its own, and inside plvs_hip_frame_extract_dev the lines of each side on another
  int n = 0, mono = -1, nl = 0, nr = 0, mono_r = -1, nlr = 0, rc_right = PLVS_OK, device = 0;
  char right_error[512] = "";
  PLVS_HIP_TRY(hipGetDevice(&device));
  std::thread right([&]() {
    if (hipSetDevice(device) != hipSuccess) {
      rc_right = PLVS_ERR_HIP;
      snprintf(right_error, sizeof right_error, "frame: hipSetDevice(%d) failed on the right image's thread", device);
      return;
    }
    rc_right = with_lines ? plvs_hip_frame_extract_dev(orb_right, lines_right, d_right, w, hh, stride, 0, 0, f->kps_right, f->desc_right,
                                                       f->kp_right_cap, &nr, &mono_r, f->keylines_right, f->line_desc_right,
                                                       f->line_right_cap, &nlr)
                          : plvs_hip_orb_extract_dev(orb_right, d_right, w, hh, stride, 0, 0, f->kps_right, f->desc_right,
                                                     f->kp_right_cap, &nr, &mono_r);
    if (rc_right != PLVS_OK) snprintf(right_error, sizeof right_error, "%s", plvs_hip_last_error());   // thread-local
  });
  const int rc_left = with_lines ? plvs_hip_frame_extract_dev(orb_left, lines_left, d_left, w, hh, stride, 0, 0, f->kps, f->desc, f->kp_cap,
                                                              &n, &mono, f->keylines, f->line_desc, f->line_cap, &nl)
                                 : plvs_hip_orb_extract_dev(orb_left, d_left, w, hh, stride, 0, 0, f->kps, f->desc, f->kp_cap, &n, &mono);
  right.join();
  if (rc_left != PLVS_OK) return rc_left;
  if (rc_right != PLVS_OK) {
    plvs::set_error("%s", right_error);
    return rc_right;
  }
  if (n > f->kp_cap || nr > f->kp_right_cap || nl > f->line_cap || nlr > f->line_right_cap) {
    plvs::set_error("frame: %d + %d key points / %d + %d lines exceed the capacities %d + %d / %d + %d", n, nr, nl, nlr, f->kp_cap,
                    f->kp_right_cap, with_lines ? f->line_cap : 0, with_lines ? f->line_right_cap : 0);
    return PLVS_ERR_CAPACITY;
  }
  f->mono_index = mono;
  f->mono_index_right = mono_r;
  if (n == 0) {   // if(mvKeys.empty()) return;  (:340-341)
    for (int c = 0; c <= kGridCells; ++c) f->cell_start[c] = 0;
    return PLVS_OK;
  }
  // 2. UndistortKeyPoints (:343)
  int rc = plvs_hip_frame_undistort_keypoints(f->kps, n, calib->K4, calib->dist, calib->ndist, f->kps_un);
  if (rc != PLVS_OK) return rc;
  // 3. ComputeStereoMatches (:345)
  int matched = 0;
  rc = plvs_hip_stereo_matches(stereo, f->kps, f->desc, n, f->kps_right, f->desc_right, nr, calib->mbf / calib->K4[0], calib->mbf,
                               f->u_right, f->depth, &matched);
  if (rc != PLVS_OK) return rc;
  // 4. UndistortKeyLines on a rectified pair (:1563-1568: mvKeyLinesUn = mvKeyLines, mvKeyLinesRightUn = mvKeyLinesRight, no
  // bounds filter, no compaction), then ComputeStereoLineMatches (:367-372)
  int stereo_lines = 0;
  if (nl > 0) {
    memcpy(f->keylines_un, f->keylines, sizeof(plvs_keyline) * (size_t)nl);
    if (nlr > 0) memcpy(f->keylines_right_un, f->keylines_right, sizeof(plvs_keyline) * (size_t)nlr);
    rc = plvs_hip_frame_compute_stereo_line_matches(f->keylines_un, f->line_desc, nl, f->keylines_right_un, f->line_desc_right, nlr,
                                                    calib->line_level_sigma2, calib->n_line_levels, calib->K4, calib->mbf,
                                                    calib->line_stereo_max_dist, calib->min_line_length_3d, calib->nn_ratio,
                                                    calib->check_orientation, calib->descriptor_dist, f->u_right_start, f->depth_start,
                                                    f->u_right_end, f->depth_end, &stereo_lines, stream);
    if (rc != PLVS_OK) return rc;
  }
  // 5. AssignFeaturesToGrid
  int items = 0;
  rc = plvs_hip_frame_assign_features_to_grid(f->kps_un, n, calib->bounds4[0], calib->bounds4[2], calib->grid_w_inv, calib->grid_h_inv,
                                              f->cell_start, f->cell_items, &items);
  if (rc != PLVS_OK) return rc;
  f->n_kp = n;
  f->n_kp_right = nr;
  f->n_lines = nl;
  f->n_lines_right = nlr;
  f->n_items = items;
  f->n_stereo_points = matched;
  f->n_stereo_lines = stereo_lines;
  return PLVS_OK;
}

}  // extern "C"
