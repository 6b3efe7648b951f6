// The local-map link of the tracking path: Frame::isInFrustum(MapPointPtr&, 0.5) and Frame::isInFrustum(MapLinePtr&, 0.5)
// (reference src/Frame.cc:955-1017, :1033-1142) over every local map point and line — the loops of
// Tracking::SearchLocalPoints / SearchLocalLines (src/Tracking.cc:4430-4579) — in ONE launch, and behind it, without a host
// wait in between, the candidate windows of ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) and
// the descriptor distances of LineMatcher::SearchByProjection(F, vpMapLines, bLargerSearch).  Single-camera frames with a
// pinhole camera (Nleft == NlinesLeft == -1); the fisheye branches (isInFrustumChecks) stay with the reference.
//
// Arithmetic: the reference's own f32 sequence in the evaluation order of Eigen 3.3 for fixed sizes — a 3x3 * 3 product row
// by row, sums of three as c0 + (c1 + c2) (dot, squaredNorm), norm = sqrt of that, Pinhole::project as fx * x / z + cx
// (a multiplication, a true division, an addition), 0.5 * (S + E) as a halving in f32.  The unit is built without
// contraction and without fast-math; `/` and sqrtf are the correctly rounded sequences (plvs_hip_selftest_walk_math).
// Only the logarithm of PredictScale cannot be had bit for bit on the device: track_level.hpp.
//
// One thread per element; the first ceil(m / 256) workgroups take a map point per thread, the others a map line.  Every
// thread posts its results straight into the pinned block (as orb_window_candidates does) and, for the one-call search,
// writes its point's window query in HBM, where orb_window_candidates — launched behind it on the same stream — reads it.
#include <cmath>
#include <cstring>
#include <optional>
#include <vector>

#include "common.hpp"
#include "line_window.hpp"
#include "orb_window.hpp"
#include "track_level.hpp"

namespace {

using plvs::orbwin::FrameGrid;
using plvs::orbwin::WinQuery;

constexpr int kPointIn = 8;     // pos[3], normal[3], mfMinDistance, mfMaxDistance
constexpr int kLineIn = 10;     // start[3], end[3], normal[3], mfMaxDistance
constexpr int kPointOut = 8;    // proj_x, proj_y, proj_xr, track_depth, view_cos, level, flags, ratio
constexpr int kLineOut = 12;    // proj[6], start_xr, end_xr, view_cos, level, flags, ratio
constexpr int kInView = 1, kAmbiguous = 2;

struct TrackParams {
  float fx, fy, cx, cy, mbf;
  float min_x, max_x, min_y, max_y;
  float R[9], t[3], Ow[3];   // mRcw in Eigen::Matrix3f's memory layout (column-major), mtcw, mOw
  float cos_limit;
  float lsf, line_lsf;       // mfLogScaleFactor, mfLineLogScaleFactor
  int levels, line_levels;
  int m, ml, point_blocks;
  int make_queries, factor, far_points;   // the one-call search: window queries of the points
  float th, th_far;
  int flip;                  // test hook: the point whose ambiguous first choice is turned to the other side (-1: none)
};

struct V3f { float x, y, z; };

__device__ __forceinline__ V3f load3(const float* p) { return V3f{p[0], p[1], p[2]}; }
__device__ __forceinline__ float dot3(const V3f& a, const V3f& b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }
__device__ __forceinline__ float norm3(const V3f& a) { return sqrtf(dot3(a, a)); }
// mRcw * P + mtcw: the product is evaluated first (a temporary), then the sum
__device__ __forceinline__ V3f to_camera(const TrackParams& P, const V3f& p) {
  const float* R = P.R;
  return V3f{(R[0] * p.x + (R[3] * p.y + R[6] * p.z)) + P.t[0], (R[1] * p.x + (R[4] * p.y + R[7] * p.z)) + P.t[1],
             (R[2] * p.x + (R[5] * p.y + R[8] * p.z)) + P.t[2]};
}
__device__ __forceinline__ float project_u(const TrackParams& P, const V3f& c) { return P.fx * c.x / c.z + P.cx; }
__device__ __forceinline__ float project_v(const TrackParams& P, const V3f& c) { return P.fy * c.y / c.z + P.cy; }

// The tests both loops share, on the point itself or on the middle of the line: depth, the four bounds (written so that a
// NaN passes, as there), the distance band, the viewing angle.  *stage: 0 rejected before the bounds test passed, 1 after.
__device__ __forceinline__ bool frustum_tests(const TrackParams& P, const V3f& world, const V3f& cam, const V3f& normal, float min_distance,
                                              float max_distance, float* u, float* v, float* dist, float* view_cos, int* stage) {
  *stage = 0;
  if (cam.z < 0.0f) return false;
  *u = project_u(P, cam);
  *v = project_v(P, cam);
  if (*u < P.min_x || *u > P.max_x) return false;
  if (*v < P.min_y || *v > P.max_y) return false;
  *stage = 1;
  const V3f PO{world.x - P.Ow[0], world.y - P.Ow[1], world.z - P.Ow[2]};
  *dist = norm3(PO);
  if (*dist < min_distance || *dist > max_distance) return false;
  if (*dist == 0.0f) return false;   // (a ratio of infinity: the level is undefined in the reference; reported as not in view)
  *view_cos = dot3(PO, normal) / *dist;
  if (*view_cos < P.cos_limit) return false;
  return true;
}

__global__ __launch_bounds__(256) void frustum_kernel(TrackParams P, const float* __restrict__ pts, const uint8_t* __restrict__ pt_skip,
                                                      const float* __restrict__ lns, const uint8_t* __restrict__ ln_skip,
                                                      const float* __restrict__ scale_factors, float* __restrict__ pt_out,
                                                      float* __restrict__ ln_out, WinQuery* __restrict__ queries) {
  if ((int)blockIdx.x < P.point_blocks) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= P.m) return;
    float px = -1.0f, py = -1.0f, pxr = 0.0f, depth = 0.0f, vcos = 0.0f, ratio = 0.0f;
    int level = 0, flags = 0;
    if (!pt_skip[k]) {
      const float* in = pts + (size_t)kPointIn * k;
      const V3f Pw = load3(in), Pn = load3(in + 3);
      const V3f Pc = to_camera(P, Pw);
      const float Pc_dist = norm3(Pc);
      const float invz = 1.0f / Pc.z;
      float u, v, dist, c;
      int stage;
      const bool ok = frustum_tests(P, Pw, Pc, Pn, 0.8f * in[6], 1.2f * in[7], &u, &v, &dist, &c, &stage);
      if (stage) { px = u; py = v; }   // (:982-983: set once the bounds test has passed, kept by the later rejections)
      if (ok) {
        ratio = in[7] / dist;
        plvs::LevelChoice lc = plvs::predict_level(ratio, P.lsf, P.levels);
        if (lc.ambiguous && k == P.flip) {
          const int nearest = (int)floor(log((double)ratio) / (double)P.lsf + 0.5);
          lc.level = lc.level == nearest ? nearest + 1 : nearest;
        }
        level = lc.level;
        flags = kInView | (lc.ambiguous ? kAmbiguous : 0);
        pxr = u - P.mbf * invz;
        depth = Pc_dist;
        vcos = c;
      }
    }
    float* o = pt_out + (size_t)kPointOut * k;
    o[0] = px; o[1] = py; o[2] = pxr; o[3] = depth; o[4] = vcos;
    o[5] = __int_as_float(level); o[6] = __int_as_float(flags); o[7] = ratio;
    if (P.make_queries) {
      const bool searched = (flags & kInView) && !(P.far_points && depth > P.th_far);
      queries[k] = searched ? plvs::orbwin::map_point_query(px, py, pxr, vcos, level, P.th, P.factor, scale_factors[level], k)
                            : WinQuery{0.0f, 0.0f, -1.0f, 0.0f, 0, 0, k, 0};   // an empty window
    }
  } else {
    const int k = ((int)blockIdx.x - P.point_blocks) * 256 + threadIdx.x;
    if (k >= P.ml) return;
    float pr[6] = {-1.0f, -1.0f, -1.0f, -1.0f, 0.0f, 0.0f};
    float sxr = -1.0f, exr = -1.0f, vcos = 0.0f, ratio = 0.0f;
    int level = 0, flags = 0;
    if (!ln_skip[k]) {
      const float* in = lns + (size_t)kLineIn * k;
      const V3f S = load3(in), E = load3(in + 3), Pn = load3(in + 6);
      const V3f Mid{(S.x + E.x) * 0.5f, (S.y + E.y) * 0.5f, (S.z + E.z) * 0.5f};
      const V3f Mc = to_camera(P, Mid);
      float u, v, dist, c;
      int stage;
      // MapLine::GetMinDistanceInvariance is 0.8f * mfMaxDistance (src/MapLine.cc:710)
      if (frustum_tests(P, Mid, Mc, Pn, 0.8f * in[9], 1.2f * in[9], &u, &v, &dist, &c, &stage)) {
        const V3f Sc = to_camera(P, S), Ec = to_camera(P, E);
        pr[0] = project_u(P, Sc); pr[1] = project_v(P, Sc);
        pr[2] = project_u(P, Ec); pr[3] = project_v(P, Ec);
        pr[4] = Sc.z; pr[5] = Ec.z;
        sxr = pr[0] - P.mbf * (1.0f / Sc.z);
        exr = pr[2] - P.mbf * (1.0f / Ec.z);
        ratio = in[9] / dist;
        const plvs::LevelChoice lc = plvs::predict_level(ratio, P.line_lsf, P.line_levels);
        level = lc.level;
        flags = kInView | (lc.ambiguous ? kAmbiguous : 0);
        vcos = c;
      }
    }
    float* o = ln_out + (size_t)kLineOut * k;
    for (int j = 0; j < 6; ++j) o[j] = pr[j];
    o[6] = sxr; o[7] = exr; o[8] = vcos;
    o[9] = __int_as_float(level); o[10] = __int_as_float(flags); o[11] = ratio;
  }
}

thread_local int g_test_flip = -1;

struct SearchArgs {
  const plvs_frame_view* F;
  const plvs_line_frame_view* LF;
  float th, th_far, nn_ratio;
  int far_points, larger_search;
  const uint8_t *occupied_points, *occupied_lines;
  int32_t* assigned_points;
  int* nmatches_points;
  int32_t* assigned_lines;
  int* nmatches_lines;
};

int check_camera(const plvs_track_camera* cam) {
  PLVS_REQUIRE(cam, "null camera");
  PLVS_REQUIRE(cam->n_cameras == 1 && cam->camera_model == PLVS_CAMERA_PINHOLE,
               "single-camera pinhole frames only (Nleft == NlinesLeft == -1): the fisheye / two-camera branches stay with the reference");
  PLVS_REQUIRE(cam->K4 && cam->bounds4 && cam->Rcw && cam->tcw && cam->Ow, "null camera / pose array");
  return PLVS_OK;
}
int check_points(const plvs_track_points* P, const plvs_track_camera* cam, bool search) {
  PLVS_REQUIRE(P->m >= 0, "negative map point count");
  if (P->m == 0) return PLVS_OK;
  PLVS_REQUIRE(cam->n_levels >= 1, "the point levels must be positive");
  PLVS_REQUIRE(P->skip && P->pos && P->normal && P->min_dist && P->max_dist, "null map point input array");
  PLVS_REQUIRE(P->in_view && P->proj_x && P->proj_y && P->proj_xr && P->track_depth && P->level && P->view_cos,
               "null map point output array");
  PLVS_REQUIRE(!search || P->desc, "null map point descriptors");
  return PLVS_OK;
}
int check_lines(const plvs_track_lines* L, const plvs_track_camera* cam, bool search) {
  PLVS_REQUIRE(L->m >= 0, "negative map line count");
  if (L->m == 0) return PLVS_OK;
  PLVS_REQUIRE(cam->n_line_levels >= 1, "the line levels must be positive");
  PLVS_REQUIRE(L->skip && L->start && L->end && L->normal && L->max_dist, "null map line input array");
  PLVS_REQUIRE(L->in_view && L->proj && L->proj_xr && L->level && L->view_cos, "null map line output array");
  PLVS_REQUIRE(!search || L->desc, "null map line descriptors");
  return PLVS_OK;
}

// ---- one call: what run() and its stages below hand on
struct Call {
  const plvs_track_points* P; const plvs_track_lines* L; const SearchArgs* S;   // the entry's arguments
  int m, ml;
  TrackParams K;
  int amb_points = 0, amb_lines = 0, levels_changed = 0, launches = 0;   // the stats
  int nv = 0, nvl = 0;                                                   // elements in view
  std::vector<int32_t> changed;                                          // points whose level the host decided otherwise
  std::vector<int32_t> q_at, q_n, pair_t, dist;                          // the points' candidates, off the staging block
};

TrackParams kernel_params(const plvs_track_camera* cam, const SearchArgs* S, int m, int ml, bool make_queries) {
  TrackParams K;
  K.fx = cam->K4[0]; K.fy = cam->K4[1]; K.cx = cam->K4[2]; K.cy = cam->K4[3]; K.mbf = cam->mbf;
  K.min_x = cam->bounds4[0]; K.max_x = cam->bounds4[1]; K.min_y = cam->bounds4[2]; K.max_y = cam->bounds4[3];
  for (int i = 0; i < 9; ++i) K.R[i] = cam->Rcw[i];
  for (int i = 0; i < 3; ++i) { K.t[i] = cam->tcw[i]; K.Ow[i] = cam->Ow[i]; }
  K.cos_limit = cam->viewing_cos_limit;
  K.lsf = cam->log_scale_factor; K.line_lsf = cam->line_log_scale_factor;
  K.levels = cam->n_levels; K.line_levels = cam->n_line_levels;
  K.m = m; K.ml = ml; K.point_blocks = (int)plvs::ceil_div((size_t)m, 256);
  K.make_queries = make_queries ? 1 : 0;
  K.th = S ? S->th : 1.0f; K.factor = (S && S->th != 1.0f) ? 1 : 0;
  K.far_points = S ? S->far_points : 0; K.th_far = S ? S->th_far : 0.0f;
  K.flip = g_test_flip;
  return K;
}

// the element inputs: kPointIn / kLineIn floats per element, and the skip flags
void pack_elements(const Call& c, float* pin, uint8_t* pskip, float* lin, uint8_t* lskip) {
  const plvs_track_points* P = c.P; const plvs_track_lines* L = c.L;
  for (int k = 0; k < c.m; ++k) {
    float* d = pin + (size_t)kPointIn * k;
    for (int j = 0; j < 3; ++j) { d[j] = P->pos[3 * (size_t)k + j]; d[3 + j] = P->normal[3 * (size_t)k + j]; }
    d[6] = P->min_dist[k]; d[7] = P->max_dist[k];
  }
  if (c.m) memcpy(pskip, P->skip, (size_t)c.m);
  for (int k = 0; k < c.ml; ++k) {
    float* d = lin + (size_t)kLineIn * k;
    for (int j = 0; j < 3; ++j) { d[j] = L->start[3 * (size_t)k + j]; d[3 + j] = L->end[3 * (size_t)k + j]; d[6 + j] = L->normal[3 * (size_t)k + j]; }
    d[9] = L->max_dist[k];
  }
  if (c.ml) memcpy(lskip, L->skip, (size_t)c.ml);
}

// after the wait: the fields, with the level of every marked element decided by the reference's expression on this process's libm
void read_fields(Call& c, const float* po, const float* lo) {
  const plvs_track_points* P = c.P; const plvs_track_lines* L = c.L;
  for (int k = 0; k < c.m; ++k) {
    const float* o = po + (size_t)kPointOut * k;
    int level, flags;
    memcpy(&level, o + 5, 4);
    memcpy(&flags, o + 6, 4);
    if (flags & kAmbiguous) {
      ++c.amb_points;
      const int host = plvs::predict_level_host(o[7], c.K.lsf, c.K.levels, 0);
      if (host != level) { level = host; c.changed.push_back(k); }
    }
    P->in_view[k] = (flags & kInView) ? 1 : 0;
    c.nv += (flags & kInView) ? 1 : 0;
    P->proj_x[k] = o[0]; P->proj_y[k] = o[1]; P->proj_xr[k] = o[2]; P->track_depth[k] = o[3]; P->view_cos[k] = o[4];
    P->level[k] = level;
  }
  for (int k = 0; k < c.ml; ++k) {
    const float* o = lo + (size_t)kLineOut * k;
    int level, flags;
    memcpy(&level, o + 9, 4);
    memcpy(&flags, o + 10, 4);
    if (flags & kAmbiguous) {
      ++c.amb_lines;
      const int host = plvs::predict_level_host(o[11], c.K.line_lsf, c.K.line_levels, 0);
      if (host != level) { level = host; ++c.levels_changed; }
    }
    L->in_view[k] = (flags & kInView) ? 1 : 0;
    c.nvl += (flags & kInView) ? 1 : 0;
    for (int j = 0; j < 6; ++j) L->proj[6 * (size_t)k + j] = o[j];
    L->proj_xr[2 * (size_t)k] = o[6]; L->proj_xr[2 * (size_t)k + 1] = o[7];
    L->view_cos[k] = o[8];
    L->level[k] = level;
  }
  c.levels_changed += (int)c.changed.size();
}

// LineMatcher::SearchByProjection(F, vpMapLines, bLargerSearch): windows and gates on the host from the fields; the distances have
// been in the matrix since the wait
int line_search(const Call& c, plvs::linewin::MatrixStage& M) {
  const SearchArgs* S = c.S;
  const plvs::linewin::LineGrid lgrid(S->LF);
  plvs::linewin::Candidates C;
  int rc = plvs::linewin::map_line_candidates(S->LF, lgrid, c.ml, c.L->in_view, c.L->proj, c.L->level, S->larger_search, C);
  if (rc != PLVS_OK) return rc;
  rc = plvs::linewin::candidate_distances(S->LF, c.L->desc, c.ml, C, M);
  if (rc != PLVS_OK) return rc;
  *S->nmatches_lines = plvs::linewin::greedy_map_lines(S->LF, c.ml, C, S->occupied_lines, c.L->has_obs, S->nn_ratio, S->assigned_lines);
  return PLVS_OK;
}

// ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) over the candidates the call's launch left — or,
// where it spilled (`found` candidates) or the host decided a level otherwise, over those of one more launch
int point_search(Call& c, const FrameGrid& grid, bool spilled, size_t found, plvs::linewin::MatrixStage& M) {
  const plvs_track_points* P = c.P; const plvs_frame_view* F = c.S->F; const TrackParams& K = c.K;
  // the windows of the points `ks` once more, from the fields the host now holds (the frustum kernel is not run again), their lists
  // appended; the launch lays out the staging block anew: the matrix leaves it first
  auto rewindow = [&](const std::vector<int32_t>& ks, size_t first_cap) -> int {
    std::vector<WinQuery> wq;
    for (int k : ks)
      if (P->in_view[k] && !(K.far_points && P->track_depth[k] > K.th_far))
        wq.push_back(plvs::orbwin::map_point_query(P->proj_x[k], P->proj_y[k], P->proj_xr[k], P->view_cos[k], P->level[k], K.th, K.factor,
                                                   F->scale_factors[P->level[k]], k));
    if (wq.empty()) return PLVS_OK;
    M.keep();
    std::vector<int32_t> qa, qn, pt2, d2;
    const int rc = plvs::orbwin::window_candidates(F, grid, wq, P->desc, c.m, qa, qn, pt2, d2, first_cap, &c.launches);
    if (rc != PLVS_OK) return rc;
    const int32_t base = (int32_t)c.pair_t.size();
    c.pair_t.insert(c.pair_t.end(), pt2.begin(), pt2.end());
    c.dist.insert(c.dist.end(), d2.begin(), d2.end());
    for (size_t j = 0; j < wq.size(); ++j) { c.q_at[wq[j].src] = base + qa[j]; c.q_n[wq[j].src] = qn[j]; }
    return PLVS_OK;
  };
  std::vector<int32_t> src((size_t)c.m);
  for (int k = 0; k < c.m; ++k) src[k] = k;
  int rc = PLVS_OK;
  if (spilled) rc = rewindow(src, found + 64);                  // more candidates than the block had room for: every window
  else if (!c.changed.empty()) rc = rewindow(c.changed, 0);     // the windows of the points with another level alone
  if (rc != PLVS_OK) return rc;
  *c.S->nmatches_points = plvs::orbwin::greedy_points(F, src.data(), (size_t)c.m, c.q_at, c.q_n, c.pair_t, c.dist, c.S->nn_ratio,
                                                     c.S->occupied_points, P->has_obs, c.S->assigned_points);
  return PLVS_OK;
}

// Both loops in one launch and, with S, the two searches behind them: one wait on the common path.
int run(const plvs_track_camera* cam, const plvs_track_points* P, const plvs_track_lines* L, const SearchArgs* S, int* n_in_view_points,
        int* n_in_view_lines, int32_t* stats, hipStream_t stream, bool own_stream) {
  Call c{P, L, S, P ? P->m : 0, L ? L->m : 0};
  const int m = c.m, ml = c.ml;
  auto finish = [&]() {
    if (n_in_view_points) *n_in_view_points = c.nv;
    if (n_in_view_lines) *n_in_view_lines = c.nvl;
    if (stats) { stats[0] = c.amb_points; stats[1] = c.amb_lines; stats[2] = c.levels_changed; stats[3] = c.launches; }
  };
  if (m == 0 && ml == 0) { finish(); return PLVS_OK; }
  const plvs_frame_view* F = S ? S->F : nullptr;
  const plvs_line_frame_view* LF = S ? S->LF : nullptr;
  const bool search_points = S && m > 0 && F->n > 0;
  const bool search_lines = S && ml > 0 && LF && LF->n > 0;
  c.K = kernel_params(cam, S, m, ml, search_points);

  // ---- one staged block: [inputs, copied in one piece | window queries, HBM only | results, posted into the pinned side]
  std::optional<FrameGrid> grid;
  plvs::orbwin::WindowStage W;
  if (search_points) W = plvs::orbwin::WindowStage{F, &grid.emplace(F), m, m, P->desc};
  plvs::linewin::MatrixStage M;
  if (search_lines) M = plvs::linewin::MatrixStage{L->desc, LF->descriptors, ml, LF->n};
  plvs::Take take;
  const size_t o_pts = take(sizeof(float) * kPointIn * (size_t)m), o_pskip = take((size_t)m);
  const size_t o_lns = take(sizeof(float) * kLineIn * (size_t)ml), o_lskip = take((size_t)ml);
  const size_t o_sf = take(search_points ? sizeof(float) * (size_t)c.K.levels : 0);
  W.take_inputs(take); M.take_inputs(take);
  const size_t in_end = take.at;
  W.take_scratch(take);
  const size_t o_pout = take(sizeof(float) * kPointOut * (size_t)m), o_lout = take(sizeof(float) * kLineOut * (size_t)ml);
  W.take_outputs(take); M.take_outputs(take);
  plvs::HostStage& st = plvs::thread_stage();
  PLVS_HIP_TRY(st.reserve(take.at + 16));
  if (own_stream) stream = st.stream;

  pack_elements(c, reinterpret_cast<float*>(st.pinned + o_pts), reinterpret_cast<uint8_t*>(st.pinned + o_pskip),
                reinterpret_cast<float*>(st.pinned + o_lns), reinterpret_cast<uint8_t*>(st.pinned + o_lskip));
  if (search_points) memcpy(st.pinned + o_sf, F->scale_factors, sizeof(float) * (size_t)c.K.levels);
  W.fill(st.pinned); M.fill(st.pinned);
  plvs::StreamGuard guard{stream};
  PLVS_HIP_TRY(hipMemcpyAsync(st.dev, st.pinned, in_end, hipMemcpyHostToDevice, stream));
  guard.armed = true;
  const int line_blocks = (int)plvs::ceil_div((size_t)ml, 256);
  hipLaunchKernelGGL(frustum_kernel, dim3(c.K.point_blocks + line_blocks), dim3(256), 0, stream, c.K,
                     reinterpret_cast<const float*>(st.dev + o_pts), reinterpret_cast<const uint8_t*>(st.dev + o_pskip),
                     reinterpret_cast<const float*>(st.dev + o_lns), reinterpret_cast<const uint8_t*>(st.dev + o_lskip),
                     reinterpret_cast<const float*>(st.dev + o_sf), reinterpret_cast<float*>(st.pinned + o_pout),
                     reinterpret_cast<float*>(st.pinned + o_lout), W.queries(st.dev));
  PLVS_KERNEL_CHECK();
  int rc = W.launch(st.dev, st.pinned, stream);   // the windows of every point, straight behind the kernel that wrote their queries
  if (rc != PLVS_OK) return rc;
  c.launches += search_points ? 1 : 0;
  if ((rc = M.launch(st.dev, st.pinned, stream)) != PLVS_OK) return rc;
  PLVS_HIP_TRY(hipStreamSynchronize(stream));   // the call's one wait
  guard.armed = false;

  read_fields(c, reinterpret_cast<const float*>(st.pinned + o_pout), reinterpret_cast<const float*>(st.pinned + o_lout));
  finish();
  if (!S) return PLVS_OK;
  // ---- the candidates of the points leave the staging block with the fields; the matrix stays until a launch wants the block (keep())
  c.q_at.assign((size_t)m, 0); c.q_n.assign((size_t)m, 0);
  size_t found = 0;
  const bool spilled = search_points && c.nv > 0 && !W.unpack(st.pinned, &found, c.q_at, c.q_n, c.pair_t, c.dist);
  if (search_lines && c.nvl > 0 && (rc = line_search(c, M)) != PLVS_OK) return rc;                            // nToMatch > 0, src/Tracking.cc:4569
  if (search_points && c.nv > 0 && (rc = point_search(c, *grid, spilled, found, M)) != PLVS_OK) return rc;    // :4475
  if (stats) stats[3] = c.launches;
  return PLVS_OK;
}

}  // namespace

extern "C" {

int plvs_hip_frame_is_in_frustum(const plvs_track_camera* cam, const plvs_track_points* points, const plvs_track_lines* lines,
                                 int* n_in_view_points, int* n_in_view_lines, int32_t* stats, void* stream) {
  int rc = check_camera(cam);
  if (rc != PLVS_OK) return rc;
  if (points && (rc = check_points(points, cam, false)) != PLVS_OK) return rc;
  if (lines && (rc = check_lines(lines, cam, false)) != PLVS_OK) return rc;
  return run(cam, points, lines, nullptr, n_in_view_points, n_in_view_lines, stats, static_cast<hipStream_t>(stream), stream == nullptr);
}

int plvs_hip_frame_search_local_map(const plvs_track_camera* cam, const plvs_frame_view* F, const plvs_line_frame_view* LF,
                                    const plvs_track_points* points, const plvs_track_lines* lines, float th, int far_points,
                                    float th_far, float nn_ratio, int larger_search, const uint8_t* occupied_points,
                                    const uint8_t* occupied_lines, int32_t* assigned_points, int* nmatches_points,
                                    int32_t* assigned_lines, int* nmatches_lines, int* n_in_view_points, int* n_in_view_lines,
                                    int32_t* stats, void* stream) {
  int rc = check_camera(cam);
  if (rc != PLVS_OK) return rc;
  PLVS_REQUIRE(F && points && nmatches_points, "null frame view / map points / match count");
  PLVS_REQUIRE(F->n >= 0 && (F->n == 0 || assigned_points), "bad frame view / null assigned array");
  PLVS_REQUIRE(F->n == 0 || points->m == 0 || (F->x && F->y && F->octave && F->u_right && F->desc && F->scale_factors), "null frame array");
  if ((rc = check_points(points, cam, F->n > 0)) != PLVS_OK) return rc;
  const int ml = lines ? lines->m : 0;
  if (lines && (rc = check_lines(lines, cam, LF != nullptr && LF->n > 0)) != PLVS_OK) return rc;
  PLVS_REQUIRE(ml == 0 || LF, "map lines without a line frame view");
  if (LF) {
    PLVS_REQUIRE(plvs::linewin::view_ok(LF), "bad line frame view");
    PLVS_REQUIRE(nmatches_lines && (LF->n == 0 || assigned_lines), "null line output");
    PLVS_REQUIRE(ml == 0 || LF->n_levels >= cam->n_line_levels, "the line frame view holds fewer levels than n_line_levels");
  }
  *nmatches_points = 0;
  for (int i = 0; i < F->n; ++i) assigned_points[i] = -1;
  if (LF) {
    *nmatches_lines = 0;
    for (int i = 0; i < LF->n; ++i) assigned_lines[i] = -1;
  } else if (nmatches_lines) {
    *nmatches_lines = 0;
  }
  const SearchArgs S{F, LF, th, th_far, nn_ratio, far_points, larger_search, occupied_points, occupied_lines, assigned_points,
                     nmatches_points, assigned_lines, nmatches_lines};
  return run(cam, points, lines, &S, n_in_view_points, n_in_view_lines, stats, static_cast<hipStream_t>(stream), stream == nullptr);
}

void plvs_hip_frame_track_test_flip(int point_index) { g_test_flip = point_index; }

}  // extern "C"
