// The motion-model link of the tracking path: the search of Tracking::TrackWithMotionModel (reference src/Tracking.cc:3615-3664)
// — ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1774-1993) and
// LineMatcher::SearchByProjection(CurrentFrame, LastFrame, bLargerSearch, bMono) (src/LineMatcher.cc:837-1230) — with the
// projection of the last frame's map points and lines on the device: Tcw * x3Dw, Pinhole::project,
// LineProjection::ProjectLineWithCheck (include/LineProjection.h:144-end) and the bounds tests in ONE launch, and behind it,
// without a host wait in between, the candidate windows of the points and the descriptor distances of the lines.
// Single-camera frames with a pinhole camera (Nleft == NlinesLeft == -1, no mpCamera2).
//
// Arithmetic: the reference's own f32 sequence.  Points: Sophus' quaternion action (track_pose.hpp), invz = the f64 quotient
// 1.0 / z rounded to f32, Pinhole::project as fx * x / z + cx — a true division, NOT a product with invz.  Lines: the middle
// 0.5 * (S + E) as a halving in f32, R p + t row by row with the product first (Eigen 3.3, fixed sizes), projectLinear, norm =
// sqrt(c0 + (c1 + c2)), invSz = 1.0f / z.  The unit is built without contraction and without fast-math; `/` and sqrtf are the
// correctly rounded sequences (plvs_hip_selftest_walk_math).  There is no logarithm on this path: nothing is decided twice.
//
// One thread per element; the first ceil(n / 256) workgroups take a last-frame point per thread, the others a last-frame line.
// Every thread posts its results straight into the pinned block and writes its point's window query in HBM, where
// orb_window_candidates — launched behind it on the same stream — reads it.
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "line_window.hpp"
#include "orb_window.hpp"
#include "track_pose.hpp"

namespace {

using plvs::orbwin::FrameGrid;
using plvs::orbwin::WinFrame;
using plvs::orbwin::WinQuery;
using plvs::trackpose::V3;

constexpr int kLineIn = 7;      // start[3], end[3], mfMaxDistance
constexpr int kPointOut = 4;    // u, v, invz, accepted
constexpr int kLineOut = 8;     // proj6, accepted, (pad)
constexpr int kMaxLevels = 64;

struct MotionParams {
  float q[4], t[3];          // Tcw: quaternion coefficients x, y, z, w and translation (the points)
  float R[9];                // mRcw in Eigen::Matrix3f's memory layout (column-major): the lines, with t
  float fx, fy, cx, cy;      // mpCamera's parameters (project)
  float lfx, lfy, lcx, lcy;  // mvLinearParameters (projectLinear)
  float mbf;
  float min_x, max_x, min_y, max_y;
  float th;
  int forward, backward;
  int n, nl, point_blocks;
  int make_queries;
};

// mRcw * P + mtcw: the product is evaluated first (a temporary), then the sum
__device__ __forceinline__ V3 to_camera(const MotionParams& P, const V3& p) {
  const float* R = P.R;
  return V3{(R[0] * p.x + (R[3] * p.y + R[6] * p.z)) + P.t[0], (R[1] * p.x + (R[4] * p.y + R[7] * p.z)) + P.t[1],
            (R[2] * p.x + (R[5] * p.y + R[8] * p.z)) + P.t[2]};
}
// the four comparisons of both functions: a NaN passes them, as there
__device__ __forceinline__ bool outside(const MotionParams& P, float u, float v) {
  if (u < P.min_x || u > P.max_x) return true;
  if (v < P.min_y || v > P.max_y) return true;
  return false;
}

__global__ __launch_bounds__(256) void motion_project_kernel(MotionParams P, const float* __restrict__ pts, const uint8_t* __restrict__ pt_valid,
                                                             const int32_t* __restrict__ pt_octave, const float* __restrict__ lns,
                                                             const uint8_t* __restrict__ ln_valid, const float* __restrict__ scale_factors,
                                                             float* __restrict__ pt_out, float* __restrict__ ln_out,
                                                             WinQuery* __restrict__ queries) {
  if ((int)blockIdx.x < P.point_blocks) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n) return;
    float u = -1.0f, v = -1.0f, invz = 0.0f;
    int ok = 0;
    if (pt_valid[i]) {
      const float* in = pts + 3 * (size_t)i;
      const V3 pc = plvs::trackpose::se3_act(P.q, P.t, V3{in[0], in[1], in[2]});   // :1806
      invz = (float)(1.0 / (double)pc.z);                                          // :1810
      if (!(invz < 0)) {                                                           // :1812
        u = P.fx * pc.x / pc.z + P.cx;                                             // Pinhole::project
        v = P.fy * pc.y / pc.z + P.cy;
        ok = outside(P, u, v) ? 0 : 1;                                             // :1817-1820
      }
    }
    float* o = pt_out + (size_t)kPointOut * i;
    o[0] = u; o[1] = v; o[2] = invz; o[3] = __int_as_float(ok);
    if (P.make_queries) {
      const int oct = pt_octave[i];   // (checked on the host for every valid point)
      queries[i] = ok ? plvs::orbwin::last_frame_query(u, v, invz, oct, P.th, scale_factors[oct], P.mbf, P.forward, P.backward, i)
                      : WinQuery{0.0f, 0.0f, -1.0f, 0.0f, 0, 0, i, 0};   // an empty window
    }
  } else {
    const int i = ((int)blockIdx.x - P.point_blocks) * 256 + threadIdx.x;
    if (i >= P.nl) return;
    float pr[6] = {-1.0f, -1.0f, -1.0f, -1.0f, 0.0f, 0.0f};
    int ok = 0;
    if (ln_valid[i]) {
      const float* in = lns + (size_t)kLineIn * i;
      const V3 S{in[0], in[1], in[2]}, E{in[3], in[4], in[5]};
      const V3 Mid{(S.x + E.x) * 0.5f, (S.y + E.y) * 0.5f, (S.z + E.z) * 0.5f};
      const V3 Mc = to_camera(P, Mid);
      do {   // ProjectLineWithCheck for a pinhole camera, in its order: every `break` is one of its `return false`
        if (Mc.z < 0.0f) break;
        const float uM = P.lfx * Mc.x / Mc.z + P.lcx, vM = P.lfy * Mc.y / Mc.z + P.lcy;
        if (outside(P, uM, vM)) break;
        const float dist = sqrtf(Mc.x * Mc.x + (Mc.y * Mc.y + Mc.z * Mc.z));
        const float max_distance = 1.2f * in[6], min_distance = 0.8f * in[6];   // MapLine::Get{Max,Min}DistanceInvariance
        if (dist < min_distance || dist > max_distance) break;
        const V3 Sc = to_camera(P, S);
        if (Sc.z < 0.0f) break;
        const V3 Ec = to_camera(P, E);
        if (Ec.z < 0.0f) break;
        pr[4] = 1.0f / Sc.z;
        pr[0] = P.lfx * Sc.x / Sc.z + P.lcx;
        pr[1] = P.lfy * Sc.y / Sc.z + P.lcy;
        if (outside(P, pr[0], pr[1])) break;
        pr[5] = 1.0f / Ec.z;
        pr[2] = P.lfx * Ec.x / Ec.z + P.lcx;
        pr[3] = P.lfy * Ec.y / Ec.z + P.lcy;
        if (outside(P, pr[2], pr[3])) break;
        ok = 1;
      } while (false);
    }
    float* o = ln_out + (size_t)kLineOut * i;
    for (int j = 0; j < 6; ++j) o[j] = pr[j];
    o[6] = __int_as_float(ok);
    o[7] = 0.0f;
  }
}


int run(const plvs_motion_poses* M, const plvs_frame_view* F, const float* cur_angle, const plvs_line_frame_view* LF,
        const plvs_motion_points* P, const plvs_motion_lines* L, const plvs_motion_policy* pol, const uint8_t* occupied_points,
        const uint8_t* occupied_lines, int32_t* assigned_points, int32_t* assigned_lines, plvs_motion_result* res, int32_t* stats,
        int levels, hipStream_t stream, bool own_stream) {
  const int n = P ? P->n : 0, nl = L ? L->n : 0;
  int st_launches = 0, st_point_retries = 0, st_line_retries = 0, st_spills = 0;
  auto post_stats = [&]() {
    if (stats) { stats[0] = st_launches; stats[1] = st_point_retries; stats[2] = st_line_retries; stats[3] = st_spills; }
  };
  // ---- the two poses decide the level bands once, on the host (:1788-1795; the line matcher's :851-860 is the same expression)
  plvs::trackpose::direction(M->q_lw, M->tlw, M->Ow, M->mb, M->mono, &res->forward, &res->backward);
  res->th_used = pol->th;
  int larger_lines = 0;
  // no points to search (no last-frame point, or a frame without key points): the reference's first search returns 0, and so does
  // its repetition at 2 * th (:3631-3640)
  auto nothing_to_search = [&]() {
    if (0 < pol->min_point_matches) {
      larger_lines = 1;
      ++st_point_retries;
      res->th_used = 2 * pol->th;
    }
  };
  if (n == 0 && nl == 0) {   // nothing to launch; the policy as below
    nothing_to_search();
    res->larger_line_search_used = larger_lines;
    post_stats();
    return PLVS_OK;
  }
  post_stats();
  const bool search_points = n > 0 && F->n > 0;
  const bool search_lines = nl > 0 && LF && LF->n > 0;
  const int N = search_points ? F->n : 0, NL = search_lines ? LF->n : 0;
  const bool matrix = search_lines && (long long)nl * NL <= plvs::linewin::kMatrixMaxPairs;
  const int direction = res->forward ? 1 : (res->backward ? 2 : 0);

  MotionParams K;
  for (int i = 0; i < 4; ++i) K.q[i] = M->q_cw[i];
  for (int i = 0; i < 3; ++i) K.t[i] = M->tcw[i];
  for (int i = 0; i < 9; ++i) K.R[i] = M->Rcw[i];
  const float* KL = M->K4_linear ? M->K4_linear : M->K4;
  K.fx = M->K4[0]; K.fy = M->K4[1]; K.cx = M->K4[2]; K.cy = M->K4[3];
  K.lfx = KL[0]; K.lfy = KL[1]; K.lcx = KL[2]; K.lcy = KL[3];
  K.mbf = M->mbf;
  K.min_x = M->bounds4[0]; K.max_x = M->bounds4[1]; K.min_y = M->bounds4[2]; K.max_y = M->bounds4[3];
  K.th = pol->th;
  K.forward = res->forward; K.backward = res->backward;
  K.n = n; K.nl = nl; K.point_blocks = (int)plvs::ceil_div((size_t)n, 256);
  K.make_queries = search_points ? 1 : 0;

  // ---- one staged block: [inputs, copied in one piece | window queries, HBM only | results, posted into the pinned side]
  std::vector<FrameGrid> grid_holder;
  if (search_points) grid_holder.emplace_back(F);
  const FrameGrid* grid = search_points ? &grid_holder[0] : nullptr;
  const size_t nm = search_points ? grid->members.size() : 0, nstart = search_points ? grid->start.size() : 0;
  const size_t out_cap = (size_t)n * 32 + 4096;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 15) & ~(size_t)15; return o; };
  const size_t o_pts = take(sizeof(float) * 3 * (size_t)n), o_pvalid = take((size_t)n), o_poct = take(sizeof(int32_t) * (size_t)n);
  const size_t o_lns = take(sizeof(float) * kLineIn * (size_t)nl), o_lvalid = take((size_t)nl);
  const size_t o_sf = take(search_points ? sizeof(float) * (size_t)levels : 0);
  const size_t o_mem = take(sizeof(FrameGrid::Member) * nm), o_start = take(sizeof(int) * nstart);
  const size_t o_ur = take(sizeof(float) * (size_t)N), o_fd = take((size_t)N * 32), o_qd = take(search_points ? (size_t)n * 32 : 0);
  const size_t o_cur = take(16);
  const size_t o_lq = take(matrix ? (size_t)nl * 32 : 0), o_lt = take(matrix ? (size_t)NL * 32 : 0);
  const size_t in_end = at;
  const size_t o_wq = take(search_points ? sizeof(WinQuery) * (size_t)n : 0);
  const size_t o_pout = take(sizeof(float) * kPointOut * (size_t)n), o_lout = take(sizeof(float) * kLineOut * (size_t)nl);
  const size_t o_first = take(search_points ? sizeof(int32_t) * (size_t)n : 0), o_count = take(search_points ? sizeof(int32_t) * (size_t)n : 0);
  const size_t o_rec = take(search_points ? sizeof(int2) * out_cap : 0);
  const size_t o_mat = take(matrix ? sizeof(uint16_t) * (size_t)nl * (size_t)NL : 0);
  plvs::HostStage& st = plvs::thread_stage();
  PLVS_HIP_TRY(st.reserve(at + 16));
  if (own_stream) stream = st.stream;

  if (n) {
    memcpy(st.pinned + o_pts, P->pos, sizeof(float) * 3 * (size_t)n);
    memcpy(st.pinned + o_pvalid, P->valid, (size_t)n);
    memcpy(st.pinned + o_poct, P->octave, sizeof(int32_t) * (size_t)n);
  }
  float* lin = reinterpret_cast<float*>(st.pinned + o_lns);
  for (int k = 0; k < nl; ++k) {
    float* d = lin + (size_t)kLineIn * k;
    for (int j = 0; j < 3; ++j) { d[j] = L->start[3 * (size_t)k + j]; d[3 + j] = L->end[3 * (size_t)k + j]; }
    d[6] = L->max_dist[k];
  }
  if (nl) memcpy(st.pinned + o_lvalid, L->valid, (size_t)nl);
  if (search_points) {
    memcpy(st.pinned + o_sf, F->scale_factors, sizeof(float) * (size_t)levels);
    memcpy(st.pinned + o_mem, grid->members.data(), sizeof(FrameGrid::Member) * nm);
    memcpy(st.pinned + o_start, grid->start.data(), sizeof(int) * nstart);
    memcpy(st.pinned + o_ur, F->u_right, sizeof(float) * (size_t)N);
    memcpy(st.pinned + o_fd, F->desc, (size_t)N * 32);
    memcpy(st.pinned + o_qd, P->desc, (size_t)n * 32);
  }
  memset(st.pinned + o_cur, 0, 16);
  if (matrix) {
    memcpy(st.pinned + o_lq, L->desc, (size_t)nl * 32);
    memcpy(st.pinned + o_lt, LF->descriptors, (size_t)NL * 32);
  }
  plvs::StreamGuard guard{stream};
  PLVS_HIP_TRY(hipMemcpyAsync(st.dev, st.pinned, in_end, hipMemcpyHostToDevice, stream));
  guard.armed = true;
  const int line_blocks = (int)plvs::ceil_div((size_t)nl, 256);
  hipLaunchKernelGGL(motion_project_kernel, dim3(K.point_blocks + line_blocks), dim3(256), 0, stream, K,
                     reinterpret_cast<const float*>(st.dev + o_pts), reinterpret_cast<const uint8_t*>(st.dev + o_pvalid),
                     reinterpret_cast<const int32_t*>(st.dev + o_poct), reinterpret_cast<const float*>(st.dev + o_lns),
                     reinterpret_cast<const uint8_t*>(st.dev + o_lvalid), reinterpret_cast<const float*>(st.dev + o_sf),
                     reinterpret_cast<float*>(st.pinned + o_pout), reinterpret_cast<float*>(st.pinned + o_lout),
                     reinterpret_cast<WinQuery*>(st.dev + o_wq));
  PLVS_KERNEL_CHECK();
  if (search_points) {   // the windows of every point, straight behind the kernel that wrote their queries
    const WinFrame wf{reinterpret_cast<const FrameGrid::Member*>(st.dev + o_mem), reinterpret_cast<const int*>(st.dev + o_start),
                      reinterpret_cast<const float*>(st.dev + o_ur), reinterpret_cast<const uint4*>(st.dev + o_fd),
                      F->min_x, F->min_y, F->grid_w_inv, F->grid_h_inv};
    hipLaunchKernelGGL(plvs::orbwin::orb_window_candidates, dim3(plvs::ceil_div((size_t)n, 4)), dim3(256), 0, stream,
                       reinterpret_cast<const WinQuery*>(st.dev + o_wq), n, wf, reinterpret_cast<const uint4*>(st.dev + o_qd),
                       reinterpret_cast<uint32_t*>(st.dev + o_cur), reinterpret_cast<int32_t*>(st.pinned + o_first),
                       reinterpret_cast<int32_t*>(st.pinned + o_count), reinterpret_cast<int2*>(st.pinned + o_rec), (uint32_t)out_cap);
    PLVS_KERNEL_CHECK();
    ++st_launches;
  }
  if (matrix) {   // depends on the descriptors alone
    hipLaunchKernelGGL(plvs::linewin::hamming_matrix_kernel, dim3(plvs::ceil_div((size_t)nl * NL, 256)), dim3(256), 0, stream,
                       reinterpret_cast<const uint4*>(st.dev + o_lq), nl, reinterpret_cast<const uint4*>(st.dev + o_lt), NL,
                       reinterpret_cast<uint16_t*>(st.pinned + o_mat));
    PLVS_KERNEL_CHECK();
  }
  PLVS_HIP_TRY(hipStreamSynchronize(stream));   // the call's one wait
  guard.armed = false;

  // ---- the projection's fields leave the staging block
  std::vector<uint8_t> pv((size_t)n), lv((size_t)nl);
  std::vector<float> pu((size_t)n), pvv((size_t)n), pz((size_t)n), proj6((size_t)nl * 6);
  const float* po = reinterpret_cast<const float*>(st.pinned + o_pout);
  for (int i = 0; i < n; ++i) {
    const float* o = po + (size_t)kPointOut * i;
    int ok;
    memcpy(&ok, o + 3, 4);
    pv[i] = (uint8_t)ok; pu[i] = o[0]; pvv[i] = o[1]; pz[i] = o[2];
  }
  const float* lo = reinterpret_cast<const float*>(st.pinned + o_lout);
  for (int i = 0; i < nl; ++i) {
    const float* o = lo + (size_t)kLineOut * i;
    int ok;
    memcpy(&ok, o + 6, 4);
    lv[i] = (uint8_t)ok;
    for (int j = 0; j < 6; ++j) proj6[6 * (size_t)i + j] = o[j];
  }
  if (n) {
    if (P->proj_valid) memcpy(P->proj_valid, pv.data(), (size_t)n);
    if (P->u) memcpy(P->u, pu.data(), sizeof(float) * (size_t)n);
    if (P->v) memcpy(P->v, pvv.data(), sizeof(float) * (size_t)n);
    if (P->invz) memcpy(P->invz, pz.data(), sizeof(float) * (size_t)n);
  }
  if (nl) {
    if (L->proj_valid) memcpy(L->proj_valid, lv.data(), (size_t)nl);
    if (L->proj6) memcpy(L->proj6, proj6.data(), sizeof(float) * 6 * (size_t)nl);
  }

  // ---- the candidates of the points, and the line distances if a repeated launch is going to reuse the block
  std::vector<int32_t> q_at((size_t)n, 0), q_n((size_t)n, 0), pair_t, dist, src((size_t)n);
  for (int i = 0; i < n; ++i) src[i] = i;
  bool spilled = false;
  size_t found = 0;
  if (search_points) {
    const int32_t* qf = reinterpret_cast<const int32_t*>(st.pinned + o_first);
    const int32_t* qc = reinterpret_cast<const int32_t*>(st.pinned + o_count);
    for (int i = 0; i < n; ++i) found += (size_t)qc[i];
    spilled = found > out_cap;
    if (!spilled) {
      const int2* rec = reinterpret_cast<const int2*>(st.pinned + o_rec);
      pair_t.resize(found);
      dist.resize(found);
      uint32_t w = 0;
      for (int i = 0; i < n; ++i) {
        q_at[i] = (int32_t)w;
        q_n[i] = qc[i];
        for (int c = 0; c < qc[i]; ++c) { pair_t[w + c] = rec[qf[i] + c].x; dist[w + c] = rec[qf[i] + c].y; }
        w += (uint32_t)qc[i];
      }
    }
  }
  const uint16_t* mat = matrix ? reinterpret_cast<const uint16_t*>(st.pinned + o_mat) : nullptr;
  std::vector<uint16_t> mat_keep;
  auto keep_matrix = [&]() {   // before anything else uses the staging block
    if (matrix && mat_keep.empty()) {
      mat_keep.assign(mat, mat + (size_t)nl * (size_t)NL);
      mat = mat_keep.data();
    }
  };

  // ---- ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono), and Tracking.cc:3631-3640
  if (search_points) {
    // the windows once more from the fields the host now holds (the projection kernel is not run again)
    auto relaunch = [&](float th, size_t first_cap) -> int {
      keep_matrix();
      std::vector<WinQuery> wq;
      for (int i = 0; i < n; ++i)
        if (pv[i]) wq.push_back(plvs::orbwin::last_frame_query(pu[i], pvv[i], pz[i], P->octave[i], th, F->scale_factors[P->octave[i]], K.mbf,
                                                               K.forward, K.backward, i));
      std::vector<int32_t> qa, qn;
      const int before = st_launches;
      const int rc = plvs::orbwin::window_candidates(F, *grid, wq, P->desc, n, qa, qn, pair_t, dist, first_cap, &st_launches);
      if (rc != PLVS_OK) return rc;
      if (st_launches - before > 1) st_spills += st_launches - before - 1;
      std::fill(q_at.begin(), q_at.end(), 0);
      std::fill(q_n.begin(), q_n.end(), 0);
      for (size_t j = 0; j < wq.size(); ++j) { q_at[wq[j].src] = qa[j]; q_n[wq[j].src] = qn[j]; }
      return PLVS_OK;
    };
    auto greedy = [&]() {
      for (int i = 0; i < N; ++i) assigned_points[i] = -1;
      return plvs::orbwin::greedy_last_frame_points(F, cur_angle, src.data(), (size_t)n, q_at, q_n, pair_t, dist, P->angle, P->has_obs,
                                                    pol->check_orientation, occupied_points, assigned_points);
    };
    if (spilled) {   // more candidates than the block had room for: once more with the room they need
      ++st_spills;
      const int rc = relaunch(pol->th, found + 64);
      if (rc != PLVS_OK) { post_stats(); return rc; }
    }
    res->nmatches_points = greedy();
    if (res->nmatches_points < pol->min_point_matches) {   // :3631
      larger_lines = 1;
      ++st_point_retries;
      res->th_used = 2 * pol->th;
      const int rc = relaunch(res->th_used, 0);
      if (rc != PLVS_OK) { post_stats(); return rc; }
      res->nmatches_points = greedy();
    }
  } else {
    nothing_to_search();
  }

  // ---- LineMatcher::SearchByProjection(CurrentFrame, LastFrame, bLargerSearch, bMono), and :3653-3662: windows and gates on the
  // host from proj6; the distances have been in the pinned block since the wait
  res->larger_line_search_used = larger_lines;
  if (search_lines) {
    const plvs::linewin::LineGrid lgrid(LF);
    auto line_search = [&](int larger, int* nmatches) -> int {
      plvs::linewin::Candidates C;
      int rc = plvs::linewin::last_frame_line_candidates(LF, lgrid, nl, lv.data(), proj6.data(), L->octave, larger, direction, C);
      if (rc != PLVS_OK) return rc;
      if (matrix) {
        C.dist.assign(C.q.size(), 0);
        for (size_t c = 0; c < C.q.size(); ++c) C.dist[c] = (int)mat[(size_t)C.q[c] * (size_t)NL + (size_t)C.t[c]];
      } else {
        plvs::linewin::MatrixJob none;
        rc = plvs::linewin::candidate_distances(LF, L->desc, nl, C, none);
        if (rc != PLVS_OK) return rc;
      }
      for (int i = 0; i < NL; ++i) assigned_lines[i] = -1;
      *nmatches = plvs::linewin::greedy_last_frame_lines(LF, nl, C, occupied_lines, L->has_obs, L->angle, pol->nn_ratio_lines,
                                                         pol->check_orientation, assigned_lines);
      return PLVS_OK;
    };
    int rc = line_search(larger_lines, &res->nmatches_lines);
    if (rc != PLVS_OK) { post_stats(); return rc; }
    if (res->nmatches_lines < pol->min_line_matches && !larger_lines) {   // :3654
      ++st_line_retries;
      res->larger_line_search_used = 1;
      rc = line_search(1, &res->nmatches_lines);
      if (rc != PLVS_OK) { post_stats(); return rc; }
    }
  } else if (nl > 0 && LF && 0 < pol->min_line_matches && !larger_lines) {
    ++st_line_retries;   // (an empty line frame: both searches return 0)
    res->larger_line_search_used = 1;
  }
  post_stats();
  return PLVS_OK;
}

}  // namespace

extern "C" {

int plvs_hip_frame_search_last_frame(const plvs_motion_poses* poses, const plvs_frame_view* F, const float* cur_angle,
                                     const plvs_line_frame_view* LF, const plvs_motion_points* points, const plvs_motion_lines* lines,
                                     const plvs_motion_policy* policy, const uint8_t* occupied_points, const uint8_t* occupied_lines,
                                     int32_t* assigned_points, int32_t* assigned_lines, plvs_motion_result* result, int32_t* stats,
                                     void* stream) {
  PLVS_REQUIRE(poses && F && points && policy && result, "null poses / frame view / points / policy / result");
  PLVS_REQUIRE(poses->n_cameras == 1 && poses->camera_model == PLVS_CAMERA_PINHOLE,
               "single-camera pinhole frames only (Nleft == NlinesLeft == -1): the fisheye / two-camera branches stay with the reference");
  PLVS_REQUIRE(poses->q_cw && poses->tcw && poses->Rcw && poses->Ow && poses->q_lw && poses->tlw && poses->bounds4 && poses->K4,
               "null pose / camera array");
  PLVS_REQUIRE(F->n >= 0 && points->n >= 0, "negative size");
  PLVS_REQUIRE(F->n == 0 || assigned_points, "null assigned array");
  int levels = 0;
  if (points->n > 0) {
    PLVS_REQUIRE(points->valid && points->pos && points->octave && points->angle && points->desc, "null last-frame point array");
    PLVS_REQUIRE(F->n == 0 || (F->x && F->y && F->octave && F->u_right && F->desc && F->scale_factors && cur_angle), "null frame array");
    for (int i = 0; i < points->n; ++i) {
      if (!points->valid[i]) continue;
      PLVS_REQUIRE(points->octave[i] >= 0, "negative octave");
      PLVS_REQUIRE(points->octave[i] < kMaxLevels, "octave of a last-frame point beyond 64 levels");
      if (points->octave[i] >= levels) levels = points->octave[i] + 1;
    }
    if (levels == 0) levels = 1;   // (no valid point: the kernel reads no scale factor, the block holds one)
  }
  const int nl = lines ? lines->n : 0;
  PLVS_REQUIRE(nl >= 0, "negative line count");
  if (nl > 0) {
    PLVS_REQUIRE(lines->valid && lines->start && lines->end && lines->max_dist && lines->octave && lines->angle && lines->desc,
                 "null last-frame line array");
    PLVS_REQUIRE(LF, "last-frame lines without a line frame view");
  }
  if (LF) {
    PLVS_REQUIRE(plvs::linewin::view_ok(LF), "bad line frame view");
    PLVS_REQUIRE(LF->n == 0 || assigned_lines, "null line output");
    for (int i = 0; i < nl; ++i)
      PLVS_REQUIRE(!lines->valid[i] || (lines->octave[i] >= 0 && lines->octave[i] < LF->n_levels),
                   "octave of a last-frame line outside the frame's levels");
  }
  // (the one scale-factor entry copied when no point is valid has to exist)
  PLVS_REQUIRE(points->n == 0 || F->n == 0 || F->scale_factors, "null scale factors");
  result->nmatches_points = 0;
  result->nmatches_lines = 0;
  result->forward = result->backward = 0;
  result->th_used = policy->th;
  result->larger_line_search_used = 0;
  for (int i = 0; i < F->n; ++i) assigned_points[i] = -1;
  if (LF)
    for (int i = 0; i < LF->n; ++i) assigned_lines[i] = -1;
  return run(poses, F, cur_angle, LF, points, nl > 0 ? lines : nullptr, policy, occupied_points, occupied_lines, assigned_points,
             assigned_lines, result, stats, levels, static_cast<hipStream_t>(stream), stream == nullptr);
}

}  // extern "C"
