// The two guided line searches Tracking runs on every frame (single-camera frames):
//   LineMatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, bLargerSearch, bMono)
//                          src/LineMatcher.cc:837-1230, called by Tracking::TrackWithMotionModel (:3653)
//   LineMatcher::SearchByProjection(Frame& F, const std::vector<MapLinePtr>&, bLargerSearch)
//                          src/LineMatcher.cc:1286-1560, called by Tracking::SearchLocalLines (:4576)
// Same split as the point searches (orb_search.hip): the candidate windows — the (theta, d) line grid
// of Frame::GetLineFeaturesInArea, src/Frame.cc:1326-1475 — and the two point-to-line gates are
// evaluated on the host for every projected line first; ALL candidate descriptor distances then go
// through one batched launch (plvs_hip_hamming_pairs); the order-dependent part — best / second best,
// ratio test, "a line that already holds an observed map line is skipped", rotation histogram — replays
// the reference's loop over those distances.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "line_window.hpp"

using namespace plvs::linewin;

extern "C" {

int plvs_hip_lines_search_by_projection_ff(const plvs_line_frame_view* F, const uint8_t* occupied, int n_last,
                                           const uint8_t* valid, const float* proj, const int32_t* octave,
                                           const float* angle, const uint8_t* desc, const uint8_t* has_obs,
                                           int larger_search, int direction, float nn_ratio, int check_orientation,
                                           int32_t* assigned, int* nmatches) {
  PLVS_REQUIRE(view_ok(F), "bad frame view");
  PLVS_REQUIRE(nmatches && (F->n == 0 || assigned), "null output");
  PLVS_REQUIRE(n_last >= 0 && (n_last == 0 || (valid && proj && octave && angle && desc)), "bad last-frame arrays");
  *nmatches = 0;
  for (int i = 0; i < F->n; ++i) assigned[i] = -1;
  if (F->n == 0 || n_last == 0) return PLVS_OK;
  const float th = larger_search ? 5.024f : 3.84f;   // kChiSquareLinePointProj(Larger), :98-99
  MatrixJob job;
  MatrixGuard guard{job};
  {
    const int rcj = matrix_begin(job, desc, n_last, F->descriptors, F->n);
    if (rcj != PLVS_OK) return rcj;
  }
  const LineGrid grid(F);
  // ---- pass 1: windows and gates for every projected line
  Candidates C;
  C.first.assign((size_t)n_last + 1, 0);
  std::vector<int> win;
  for (int i = 0; i < n_last; ++i) {
    C.first[(size_t)i] = (int)C.q.size();
    if (!valid[i]) continue;
    const float* p = proj + 6 * (size_t)i;
    const Rep pr = representation(p[0], p[1], p[2], p[3]);
    const int lo = octave[i];
    PLVS_REQUIRE(lo >= 0 && lo < F->n_levels, "octave of a last-frame line outside the frame's levels");
    const float sc = F->line_scale_factors[lo];
    const float dtheta = (float)(10 * M_PI / 180.f) * sc, dd = 100.0f * sc;   // Frame::kDeltaTheta, kDeltaD
    bool ok;
    if (direction == 1) ok = grid.search(pr, dtheta, dd, lo, 2147483647, win);        // bForward
    else if (direction == 2) ok = grid.search(pr, dtheta, dd, 0, lo, win);            // bBackward
    else ok = grid.search(pr, dtheta, dd, lo - 1, lo + 1, win);
    if (!ok) {
      plvs::set_error("GetLineFeaturesInArea: search over the full theta interval (the reference terminates here)");
      return PLVS_ERR_INVALID_ARG;
    }
    RightRep rr;
    for (int i2 : win)
      if (passes_gates(F, i2, pr, F->line_inv_level_sigma2[lo], th, p, F->bf * p[4], F->bf * p[5], rr)) {
        C.q.push_back(i);
        C.t.push_back(i2);
      }
  }
  C.first[(size_t)n_last] = (int)C.q.size();
  // ---- all candidate distances in one launch
  const int rc = candidate_distances(F, desc, n_last, C, job);
  if (rc != PLVS_OK) return rc;
  // ---- pass 2: the reference's loop
  std::vector<uint8_t> occ((size_t)F->n, 0);
  if (occupied)
    for (int i = 0; i < F->n; ++i) occ[(size_t)i] = occupied[i];
  const float factor = (float)(kHisto / (2.0 * M_PI));
  std::vector<int> pushed, pushed_bin;
  int n = 0;
  for (int i = 0; i < n_last; ++i) {
    int best = 256, best2 = 256, best_idx = -1;
    for (int c = C.first[(size_t)i]; c < C.first[(size_t)i + 1]; ++c) {
      const int i2 = C.t[(size_t)c];
      if (occ[(size_t)i2]) continue;
      const int d = C.dist[(size_t)c];
      if (d < best) { best2 = best; best = d; best_idx = i2; }
      else if (d < best2) { best2 = d; }
    }
    if (best <= kThHigh && best_idx >= 0) {
      if ((float)best > nn_ratio * (float)best2) continue;
      assigned[best_idx] = i;
      occ[(size_t)best_idx] = has_obs ? has_obs[i] : 1;
      ++n;
      if (check_orientation) {
        float rot = angle[i] - F->keylines_un[best_idx].angle;
        if (rot < 0.0) rot += (float)(2.0 * M_PI); else if (rot > (float)(2.0 * M_PI)) rot -= (float)(2.0 * M_PI);
        int bin = (int)std::round(rot * factor);
        if (bin == kHisto) bin = 0;
        pushed.push_back(best_idx);
        pushed_bin.push_back(bin);
      }
    }
  }
  if (check_orientation) {   // ComputeThreeMaxima (:101-145) and the cut of the other bins (:1215-1225)
    int cnt[kHisto] = {0};
    for (int b : pushed_bin) ++cnt[b];
    int i1 = -1, i2 = -1, i3 = -1, m1 = 0, m2 = 0, m3 = 0;
    for (int b = 0; b < kHisto; ++b) {
      const int s = cnt[b];
      if (s > m1) { m3 = m2; m2 = m1; m1 = s; i3 = i2; i2 = i1; i1 = b; }
      else if (s > m2) { m3 = m2; m2 = s; i3 = i2; i2 = b; }
      else if (s > m3) { m3 = s; i3 = b; }
    }
    if (m2 < 0.1f * (float)m1) { i2 = -1; i3 = -1; }
    else if (m3 < 0.1f * (float)m1) { i3 = -1; }
    for (size_t k = 0; k < pushed.size(); ++k)
      if (pushed_bin[k] != i1 && pushed_bin[k] != i2 && pushed_bin[k] != i3) {
        assigned[pushed[k]] = -1;
        --n;
      }
  }
  *nmatches = n;
  return PLVS_OK;
}

int plvs_hip_lines_search_by_projection(const plvs_line_frame_view* F, const uint8_t* occupied, int n_map,
                                        const uint8_t* in_view, const float* proj, const int32_t* level,
                                        const uint8_t* desc, const uint8_t* has_obs, int larger_search,
                                        float nn_ratio, int32_t* assigned, int* nmatches) {
  PLVS_REQUIRE(view_ok(F), "bad frame view");
  PLVS_REQUIRE(nmatches && (F->n == 0 || assigned), "null output");
  PLVS_REQUIRE(n_map >= 0 && (n_map == 0 || (in_view && proj && level && desc)), "bad map-line arrays");
  *nmatches = 0;
  for (int i = 0; i < F->n; ++i) assigned[i] = -1;
  if (F->n == 0 || n_map == 0) return PLVS_OK;
  MatrixJob job;
  MatrixGuard guard{job};
  {
    const int rcj = matrix_begin(job, desc, n_map, F->descriptors, F->n);
    if (rcj != PLVS_OK) return rcj;
  }
  const LineGrid grid(F);
  Candidates C;
  int rc = map_line_candidates(F, grid, n_map, in_view, proj, level, larger_search, C);
  if (rc != PLVS_OK) return rc;
  rc = candidate_distances(F, desc, n_map, C, job);
  if (rc != PLVS_OK) return rc;
  const int n = greedy_map_lines(F, n_map, C, occupied, has_obs, nn_ratio, assigned);
  *nmatches = n;
  return PLVS_OK;
}

}  // extern "C"
