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
  MatrixJob job;
  MatrixGuard guard{job};
  {
    const int rcj = matrix_begin(job, desc, n_last, F->descriptors, F->n);
    if (rcj != PLVS_OK) return rcj;
  }
  const LineGrid grid(F);
  // ---- pass 1: windows and gates for every projected line
  Candidates C;
  int rc = last_frame_line_candidates(F, grid, n_last, valid, proj, octave, larger_search, direction, C);
  if (rc != PLVS_OK) return rc;
  // ---- all candidate distances in one launch
  rc = candidate_distances(F, desc, n_last, C, job);
  if (rc != PLVS_OK) return rc;
  // ---- pass 2: the reference's loop
  *nmatches = greedy_last_frame_lines(F, n_last, C, occupied, has_obs, angle, nn_ratio, check_orientation, assigned);
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
