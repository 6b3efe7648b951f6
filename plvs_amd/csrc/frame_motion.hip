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
#include <optional>
#include <vector>

#include "common.hpp"
#include "line_window.hpp"
#include "orb_window.hpp"
#include "track_pose.hpp"

namespace {

using plvs::orbwin::FrameGrid;
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

// ---- one call: what run() and its stages below hand on
struct Call {
  const plvs_frame_view* F; const float* cur_angle; const plvs_line_frame_view* LF;   // the entry's arguments
  const plvs_motion_points* P; const plvs_motion_lines* L; const plvs_motion_policy* pol;
  const uint8_t *occupied_points, *occupied_lines;
  int32_t *assigned_points, *assigned_lines;
  plvs_motion_result* res;
  int n, nl;
  MotionParams K;
  int launches = 0, point_retries = 0, line_retries = 0, spills = 0;   // the stats
  int larger_lines = 0;                                                // bLargerLineSearch after the points (:3636)
  std::vector<uint8_t> pv, lv;                                         // the projection's fields, off the staging block
  std::vector<float> pu, pvv, pz, proj6;
  std::vector<int32_t> q_at, q_n, pair_t, dist;                        // the points' candidates, off the staging block
};

MotionParams kernel_params(const plvs_motion_poses* M, const Call& c, bool make_queries) {
  MotionParams K;
  for (int i = 0; i < 4; ++i) K.q[i] = M->q_cw[i];
  for (int i = 0; i < 3; ++i) K.t[i] = M->tcw[i];
  for (int i = 0; i < 9; ++i) K.R[i] = M->Rcw[i];
  const float* KL = M->K4_linear ? M->K4_linear : M->K4;
  K.fx = M->K4[0]; K.fy = M->K4[1]; K.cx = M->K4[2]; K.cy = M->K4[3];
  K.lfx = KL[0]; K.lfy = KL[1]; K.lcx = KL[2]; K.lcy = KL[3];
  K.mbf = M->mbf;
  K.min_x = M->bounds4[0]; K.max_x = M->bounds4[1]; K.min_y = M->bounds4[2]; K.max_y = M->bounds4[3];
  K.th = c.pol->th;
  K.forward = c.res->forward; K.backward = c.res->backward;
  K.n = c.n; K.nl = c.nl; K.point_blocks = (int)plvs::ceil_div((size_t)c.n, 256);
  K.make_queries = make_queries ? 1 : 0;
  return K;
}

// the element inputs: the points' arrays as they are, kLineIn floats per line, and the valid flags
void pack_elements(const Call& c, char* pts, char* pvalid, char* poct, float* lin, char* lvalid) {
  const plvs_motion_points* P = c.P; const plvs_motion_lines* L = c.L;
  if (c.n) {
    memcpy(pts, P->pos, sizeof(float) * 3 * (size_t)c.n);
    memcpy(pvalid, P->valid, (size_t)c.n);
    memcpy(poct, P->octave, sizeof(int32_t) * (size_t)c.n);
  }
  for (int k = 0; k < c.nl; ++k) {
    float* d = lin + (size_t)kLineIn * k;
    for (int j = 0; j < 3; ++j) { d[j] = L->start[3 * (size_t)k + j]; d[3 + j] = L->end[3 * (size_t)k + j]; }
    d[6] = L->max_dist[k];
  }
  if (c.nl) memcpy(lvalid, L->valid, (size_t)c.nl);
}

// after the wait: the projection's fields leave the staging block, for the searches and for the caller
void read_fields(Call& c, const float* po, const float* lo) {
  const int n = c.n, nl = c.nl;
  c.pv.resize((size_t)n); c.pu.resize((size_t)n); c.pvv.resize((size_t)n); c.pz.resize((size_t)n);
  c.lv.resize((size_t)nl); c.proj6.resize((size_t)nl * 6);
  for (int i = 0; i < n; ++i) {
    const float* o = po + (size_t)kPointOut * i;
    int ok;
    memcpy(&ok, o + 3, 4);
    c.pv[i] = (uint8_t)ok; c.pu[i] = o[0]; c.pvv[i] = o[1]; c.pz[i] = o[2];
  }
  for (int i = 0; i < nl; ++i) {
    const float* o = lo + (size_t)kLineOut * i;
    int ok;
    memcpy(&ok, o + 6, 4);
    c.lv[i] = (uint8_t)ok;
    for (int j = 0; j < 6; ++j) c.proj6[6 * (size_t)i + j] = o[j];
  }
  if (n) {
    if (c.P->proj_valid) memcpy(c.P->proj_valid, c.pv.data(), (size_t)n);
    if (c.P->u) memcpy(c.P->u, c.pu.data(), sizeof(float) * (size_t)n);
    if (c.P->v) memcpy(c.P->v, c.pvv.data(), sizeof(float) * (size_t)n);
    if (c.P->invz) memcpy(c.P->invz, c.pz.data(), sizeof(float) * (size_t)n);
  }
  if (nl) {
    if (c.L->proj_valid) memcpy(c.L->proj_valid, c.lv.data(), (size_t)nl);
    if (c.L->proj6) memcpy(c.L->proj6, c.proj6.data(), sizeof(float) * 6 * (size_t)nl);
  }
}

// no points to search (no last-frame point, or a frame without key points): the reference's first search returns 0, and so does
// its repetition at 2 * th (:3631-3640)
void nothing_to_search(Call& c) {
  if (0 < c.pol->min_point_matches) { c.larger_lines = 1; ++c.point_retries; c.res->th_used = 2 * c.pol->th; }
}

// ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) over the candidates the call's launch left (or, where it spilled
// with `found` candidates, over those of one more launch), and Tracking.cc:3631-3640
int point_search(Call& c, const FrameGrid& grid, bool spilled, size_t found, plvs::linewin::MatrixStage& M) {
  const plvs_motion_points* P = c.P; const plvs_frame_view* F = c.F;
  const int n = c.n;
  std::vector<int32_t> src((size_t)n);
  for (int i = 0; i < n; ++i) src[i] = i;
  // the windows once more from the fields the host now holds (the projection kernel is not run again); the launch lays out the
  // staging block anew: the matrix leaves it first
  auto relaunch = [&](float th, size_t first_cap) -> int {
    M.keep();
    std::vector<WinQuery> wq;
    for (int i = 0; i < n; ++i)
      if (c.pv[i]) wq.push_back(plvs::orbwin::last_frame_query(c.pu[i], c.pvv[i], c.pz[i], P->octave[i], th, F->scale_factors[P->octave[i]],
                                                               c.K.mbf, c.K.forward, c.K.backward, i));
    std::vector<int32_t> qa, qn;
    const int before = c.launches;
    const int rc = plvs::orbwin::window_candidates(F, grid, wq, P->desc, n, qa, qn, c.pair_t, c.dist, first_cap, &c.launches);
    if (rc != PLVS_OK) return rc;
    if (c.launches - before > 1) c.spills += c.launches - before - 1;
    std::fill(c.q_at.begin(), c.q_at.end(), 0);
    std::fill(c.q_n.begin(), c.q_n.end(), 0);
    for (size_t j = 0; j < wq.size(); ++j) { c.q_at[wq[j].src] = qa[j]; c.q_n[wq[j].src] = qn[j]; }
    return PLVS_OK;
  };
  auto greedy = [&]() {
    for (int i = 0; i < F->n; ++i) c.assigned_points[i] = -1;
    return plvs::orbwin::greedy_last_frame_points(F, c.cur_angle, src.data(), (size_t)n, c.q_at, c.q_n, c.pair_t, c.dist, P->angle, P->has_obs,
                                                  c.pol->check_orientation, c.occupied_points, c.assigned_points);
  };
  if (spilled) {   // more candidates than the block had room for: once more with the room they need
    ++c.spills;
    const int rc = relaunch(c.pol->th, found + 64);
    if (rc != PLVS_OK) return rc;
  }
  c.res->nmatches_points = greedy();
  if (c.res->nmatches_points < c.pol->min_point_matches) {   // :3631
    c.larger_lines = 1;
    ++c.point_retries;
    c.res->th_used = 2 * c.pol->th;
    const int rc = relaunch(c.res->th_used, 0);
    if (rc != PLVS_OK) return rc;
    c.res->nmatches_points = greedy();
  }
  return PLVS_OK;
}

// LineMatcher::SearchByProjection(CurrentFrame, LastFrame, bLargerSearch, bMono), and :3653-3662: windows and gates on the host from
// proj6; the distances have been in the matrix since the wait
int line_search(Call& c, bool search_lines, int direction, plvs::linewin::MatrixStage& M) {
  const plvs_motion_lines* L = c.L; const plvs_line_frame_view* LF = c.LF;
  c.res->larger_line_search_used = c.larger_lines;
  if (!search_lines) {   // (an empty line frame: both searches return 0)
    if (c.nl > 0 && LF && 0 < c.pol->min_line_matches && !c.larger_lines) { ++c.line_retries; c.res->larger_line_search_used = 1; }
    return PLVS_OK;
  }
  const plvs::linewin::LineGrid lgrid(LF);
  auto search = [&](int larger) -> int {
    plvs::linewin::Candidates C;
    int rc = plvs::linewin::last_frame_line_candidates(LF, lgrid, c.nl, c.lv.data(), c.proj6.data(), L->octave, larger, direction, C);
    if (rc != PLVS_OK) return rc;
    rc = plvs::linewin::candidate_distances(LF, L->desc, c.nl, C, M);
    if (rc != PLVS_OK) return rc;
    for (int i = 0; i < LF->n; ++i) c.assigned_lines[i] = -1;
    c.res->nmatches_lines = plvs::linewin::greedy_last_frame_lines(LF, c.nl, C, c.occupied_lines, L->has_obs, L->angle, c.pol->nn_ratio_lines,
                                                                  c.pol->check_orientation, c.assigned_lines);
    return PLVS_OK;
  };
  int rc = search(c.larger_lines);
  if (rc == PLVS_OK && c.res->nmatches_lines < c.pol->min_line_matches && !c.larger_lines) {   // :3654
    ++c.line_retries;
    c.res->larger_line_search_used = 1;
    rc = search(1);
  }
  return rc;
}

int run(const plvs_motion_poses* M, const plvs_frame_view* F, const float* cur_angle, const plvs_line_frame_view* LF,
        const plvs_motion_points* P, const plvs_motion_lines* L, const plvs_motion_policy* pol, const uint8_t* occupied_points,
        const uint8_t* occupied_lines, int32_t* assigned_points, int32_t* assigned_lines, plvs_motion_result* res, int32_t* stats,
        int levels, hipStream_t stream, bool own_stream) {
  Call c{F, cur_angle, LF, P, L, pol, occupied_points, occupied_lines, assigned_points, assigned_lines, res, P ? P->n : 0, L ? L->n : 0};
  const int n = c.n, nl = c.nl;
  auto post_stats = [&]() {
    if (stats) { stats[0] = c.launches; stats[1] = c.point_retries; stats[2] = c.line_retries; stats[3] = c.spills; }
  };
  // ---- the two poses decide the level bands once, on the host (:1788-1795; the line matcher's :851-860 is the same expression)
  plvs::trackpose::direction(M->q_lw, M->tlw, M->Ow, M->mb, M->mono, &res->forward, &res->backward);
  res->th_used = pol->th;
  if (n == 0 && nl == 0) {   // nothing to launch; the policy as below
    nothing_to_search(c);
    res->larger_line_search_used = c.larger_lines;
    post_stats();
    return PLVS_OK;
  }
  post_stats();
  const bool search_points = n > 0 && F->n > 0;
  const bool search_lines = nl > 0 && LF && LF->n > 0;
  const int direction = res->forward ? 1 : (res->backward ? 2 : 0);
  c.K = kernel_params(M, c, search_points);

  // ---- one staged block: [inputs, copied in one piece | window queries, HBM only | results, posted into the pinned side]
  std::optional<FrameGrid> grid;
  plvs::orbwin::WindowStage W;
  if (search_points) W = plvs::orbwin::WindowStage{F, &grid.emplace(F), n, n, P->desc};
  plvs::linewin::MatrixStage X;
  if (search_lines) X = plvs::linewin::MatrixStage{L->desc, LF->descriptors, nl, LF->n};
  plvs::Take take;
  const size_t o_pts = take(sizeof(float) * 3 * (size_t)n), o_pvalid = take((size_t)n), o_poct = take(sizeof(int32_t) * (size_t)n);
  const size_t o_lns = take(sizeof(float) * kLineIn * (size_t)nl), o_lvalid = take((size_t)nl);
  const size_t o_sf = take(search_points ? sizeof(float) * (size_t)levels : 0);
  W.take_inputs(take); X.take_inputs(take);
  const size_t in_end = take.at;
  W.take_scratch(take);
  const size_t o_pout = take(sizeof(float) * kPointOut * (size_t)n), o_lout = take(sizeof(float) * kLineOut * (size_t)nl);
  W.take_outputs(take); X.take_outputs(take);
  plvs::HostStage& st = plvs::thread_stage();
  PLVS_HIP_TRY(st.reserve(take.at + 16));
  if (own_stream) stream = st.stream;

  pack_elements(c, st.pinned + o_pts, st.pinned + o_pvalid, st.pinned + o_poct, reinterpret_cast<float*>(st.pinned + o_lns), st.pinned + o_lvalid);
  if (search_points) memcpy(st.pinned + o_sf, F->scale_factors, sizeof(float) * (size_t)levels);
  W.fill(st.pinned); X.fill(st.pinned);
  plvs::StreamGuard guard{stream};
  PLVS_HIP_TRY(hipMemcpyAsync(st.dev, st.pinned, in_end, hipMemcpyHostToDevice, stream));
  guard.armed = true;
  const int line_blocks = (int)plvs::ceil_div((size_t)nl, 256);
  hipLaunchKernelGGL(motion_project_kernel, dim3(c.K.point_blocks + line_blocks), dim3(256), 0, stream, c.K,
                     reinterpret_cast<const float*>(st.dev + o_pts), reinterpret_cast<const uint8_t*>(st.dev + o_pvalid),
                     reinterpret_cast<const int32_t*>(st.dev + o_poct), reinterpret_cast<const float*>(st.dev + o_lns),
                     reinterpret_cast<const uint8_t*>(st.dev + o_lvalid), reinterpret_cast<const float*>(st.dev + o_sf),
                     reinterpret_cast<float*>(st.pinned + o_pout), reinterpret_cast<float*>(st.pinned + o_lout), W.queries(st.dev));
  PLVS_KERNEL_CHECK();
  int rc = W.launch(st.dev, st.pinned, stream);   // the windows of every point, straight behind the kernel that wrote their queries
  if (rc != PLVS_OK) return rc;
  c.launches += search_points ? 1 : 0;
  if ((rc = X.launch(st.dev, st.pinned, stream)) != PLVS_OK) return rc;
  PLVS_HIP_TRY(hipStreamSynchronize(stream));   // the call's one wait
  guard.armed = false;

  // ---- the fields and the candidates of the points leave the staging block; the matrix stays until a launch wants the block (keep())
  read_fields(c, reinterpret_cast<const float*>(st.pinned + o_pout), reinterpret_cast<const float*>(st.pinned + o_lout));
  c.q_at.assign((size_t)n, 0); c.q_n.assign((size_t)n, 0);
  size_t found = 0;
  const bool spilled = search_points && !W.unpack(st.pinned, &found, c.q_at, c.q_n, c.pair_t, c.dist);
  if (search_points) rc = point_search(c, *grid, spilled, found, X);
  else nothing_to_search(c);
  if (rc == PLVS_OK) rc = line_search(c, search_lines, direction, X);
  post_stats();
  return rc;
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
