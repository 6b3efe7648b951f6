// Key frames resident in HBM (keyframe_handle.hpp): the handle's life cycle, and the three Fuse searches of
// LocalMapping::SearchInNeighbors over handles.  A handle is created where the KeyFrame constructor ends — one reserve of the
// calling thread's staging block, one copy, one wait — and from then on a search carries the poses, the map points or lines and
// `skip`: the per-call grid build, staging and copy of every target key frame (76 % of the point call) are gone.  The
// kernels are orb_fuse.hip's and line_fuse.hip's resident ones, the call is fuse_both.hip's run_parts: one reserve, one copy in, one
// launch per kind, one wait.  The Sim3 Fuse searches of LoopClosing::SearchAndFuse (the _loop_ entries) are the same parts with
// the other gate and a plvs_keyframe_sim3_pose per key frame.
#include "fuse_jobs.hpp"
#include "keyframe_handle.hpp"

namespace fj = plvs::fusejob;

int plvs::fusejob::check_handles(const plvs_keyframe* const* kfs, const void* poses, int n_kfs, int side, bool host_entry) {
  PLVS_REQUIRE(n_kfs == 0 || poses, "null poses");
  for (int k = 0; k < n_kfs; ++k) {
    PLVS_REQUIRE(kfs[k], "null key-frame handle in the list");
    PLVS_REQUIRE(!(side & 1) || kfs[k]->pt.present, "a key-frame handle without a point side in a point search");
    PLVS_REQUIRE(!(side & 2) || kfs[k]->ln.present, "a key-frame handle without a line side in a line search");
  }
  if (host_entry) return PLVS_OK;
  for (int k = 0; k < n_kfs; ++k)
    PLVS_REQUIRE(!(kfs[k]->flags & PLVS_KEYFRAME_HOST_ONLY), "a PLVS_KEYFRAME_HOST_ONLY handle in a device entry (the _kf_host entries take it)");
  if (n_kfs == 0) return PLVS_OK;
  int device = -1;
  PLVS_HIP_TRY(hipGetDevice(&device));
  for (int k = 0; k < n_kfs; ++k) PLVS_REQUIRE(kfs[k]->device == device, "a key-frame handle created on another device than the current one");
  return PLVS_OK;
}

extern "C" {

int plvs_hip_keyframe_create(const plvs_fuse_keyframe* points, const plvs_line_fuse_keyframe* lines, uint32_t flags, plvs_keyframe** out) {
  return plvs_hip_keyframe_create_bow(points, lines, nullptr, flags, out);
}

int plvs_hip_keyframe_create_bow(const plvs_fuse_keyframe* points, const plvs_line_fuse_keyframe* lines, const plvs_keyframe_bow* bow,
                                 uint32_t flags, plvs_keyframe** out) {
  PLVS_REQUIRE(out, "null out");
  *out = nullptr;
  PLVS_REQUIRE((flags & ~PLVS_KEYFRAME_HOST_ONLY) == 0, "unknown flag");
  PLVS_REQUIRE(points || lines, "neither a point side nor a line side");
  if (points) {
    const int rc = plvs::kfhandle::check_point_keyframe(*points, false);
    if (rc != PLVS_OK) return rc;
  }
  if (lines) {
    const int rc = plvs::kfhandle::check_line_keyframe(*lines, false);
    if (rc != PLVS_OK) return rc;
  }
  int bow_listed = 0, bow_longest = 0;
  if (bow) {
    PLVS_REQUIRE(points, "a BoW side needs the point side");
    const int rc = plvs::kfhandle::check_bow(*bow, points->view.n, &bow_listed, &bow_longest);
    if (rc != PLVS_OK) return rc;
  }
  std::unique_ptr<plvs_keyframe> h(new plvs_keyframe);
  h->flags = flags;
  if (points) plvs::kfhandle::stage_points(*points, h.get());
  if (lines) plvs::kfhandle::stage_lines(*lines, h.get());
  if (bow) plvs::kfhandle::stage_bow(*bow, bow_listed, bow_longest, h.get());
  if (!(flags & PLVS_KEYFRAME_HOST_ONLY)) {
    const size_t bytes = h->host.size();
    PLVS_HIP_TRY(hipGetDevice(&h->device));
    plvs::HostStage& st = plvs::thread_stage();
    PLVS_HIP_TRY(st.reserve(bytes));
    memcpy(st.pinned, h->host.data(), bytes);
    PLVS_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->dev), bytes));
    hipError_t e = hipMemcpyAsync(h->dev, st.pinned, bytes, hipMemcpyHostToDevice, st.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(st.stream);
    if (e != hipSuccess) {
      (void)hipFree(h->dev);
      plvs::set_error("plvs_hip_keyframe_create: the copy in failed: %s", hipGetErrorString(e));
      return PLVS_ERR_HIP;
    }
  }
  *out = h.release();
  return PLVS_OK;
}

int plvs_hip_keyframe_destroy(plvs_keyframe* kf) {
  if (!kf) return PLVS_OK;
  hipError_t e = hipSuccess;
  if (kf->dev) e = hipFree(kf->dev);
  delete kf;
  PLVS_HIP_TRY(e);
  return PLVS_OK;
}

int plvs_hip_keyframe_info(const plvs_keyframe* kf, int64_t* info) {
  PLVS_REQUIRE(kf && info, "null handle / info");
  info[0] = kf->pt.present ? kf->pt.n : -1;
  info[1] = kf->ln.present ? kf->ln.n : -1;
  info[2] = kf->dev ? (int64_t)kf->host.size() : 0;
  info[3] = (int64_t)kf->host.size();
  info[4] = kf->flags;
  info[5] = kf->device;
  return PLVS_OK;
}

int plvs_hip_keyframe_bow_info(const plvs_keyframe* kf, int64_t* info) {
  PLVS_REQUIRE(kf && info, "null handle / info");
  info[0] = kf->bow.present ? kf->bow.nnodes : -1;
  info[1] = kf->bow.listed;
  info[2] = kf->bow.longest;
  info[3] = kf->dev ? (int64_t)kf->bow.bytes : 0;
  return PLVS_OK;
}

int plvs_hip_orb_fuse_search_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_pose* poses, int n_kfs, const plvs_fuse_points* P,
                                const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats,
                                void* stream) {
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_point_part_kf(kfs, poses, n_kfs, P, skip, th, best_idx, best_dist, reached, stats, false, &part);
  return rc != PLVS_OK ? rc : fj::run_single(part.get(), stats, 4, stream, false);
}

int plvs_hip_line_fuse_search_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_pose* poses, int n_kfs, const plvs_fuse_lines* L,
                                 const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats,
                                 void* stream) {
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_line_part_kf(kfs, poses, n_kfs, L, skip, th, best_idx, best_dist, reached, stats, false, &part);
  return rc != PLVS_OK ? rc : fj::run_single(part.get(), stats, 4, stream, false);
}

int plvs_hip_orb_fuse_search_kf_host(const plvs_keyframe* const* kfs, const plvs_keyframe_pose* poses, int n_kfs, const plvs_fuse_points* P,
                                     const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats) {
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_point_part_kf(kfs, poses, n_kfs, P, skip, th, best_idx, best_dist, reached, stats, true, &part);
  return rc != PLVS_OK ? rc : fj::run_single(part.get(), stats, 4, nullptr, true);
}

int plvs_hip_line_fuse_search_kf_host(const plvs_keyframe* const* kfs, const plvs_keyframe_pose* poses, int n_kfs, const plvs_fuse_lines* L,
                                      const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats) {
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_line_part_kf(kfs, poses, n_kfs, L, skip, th, best_idx, best_dist, reached, stats, true, &part);
  return rc != PLVS_OK ? rc : fj::run_single(part.get(), stats, 4, nullptr, true);
}

}  // extern "C"

// the combined entry over handles, SE3 (poses) or Sim3 (sim3): one of the two is null
static int both_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_pose* poses, const plvs_keyframe_sim3_pose* sim3, int n_kfs,
                   const plvs_fuse_points* P, const uint8_t* skip_points, float th_points, int32_t* point_best_idx, int32_t* point_best_dist,
                   uint8_t* point_reached, int32_t* point_stats, const plvs_fuse_lines* L, const uint8_t* skip_lines, float th_lines,
                   int32_t* line_best_idx, int32_t* line_best_dist, uint8_t* line_reached, int32_t* line_stats, int32_t* stats, void* stream) {
  PLVS_REQUIRE(P || L, "neither points nor lines");
  std::unique_ptr<fj::Part> points, lines;
  if (P) {   // both kinds' refusals before anything is launched or written
    const int rc = fj::make_point_part_kf(kfs, poses, n_kfs, P, skip_points, th_points, point_best_idx, point_best_dist, point_reached,
                                          point_stats, false, &points, sim3);
    if (rc != PLVS_OK) return rc;
  }
  if (L) {
    const int rc = fj::make_line_part_kf(kfs, poses, n_kfs, L, skip_lines, th_lines, line_best_idx, line_best_dist, line_reached, line_stats,
                                         false, &lines, sim3);
    if (rc != PLVS_OK) return rc;
  }
  if (P && point_stats) point_stats[0] = point_stats[1] = point_stats[2] = point_stats[3] = 0;
  if (L && line_stats) line_stats[0] = line_stats[1] = line_stats[2] = line_stats[3] = 0;
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  int launches = 0, waits = 0;
  size_t copied = 0;
  const int rc = fj::run_parts(points.get(), lines.get(), static_cast<hipStream_t>(stream), stream == nullptr, false, &launches, &waits, &copied);
  if (stats) { stats[0] = launches; stats[1] = waits; stats[2] = (int32_t)copied; }
  return rc;
}

extern "C" {

int plvs_hip_fuse_search_points_and_lines_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_pose* poses, int n_kfs,
                                             const plvs_fuse_points* P, const uint8_t* skip_points, float th_points, int32_t* point_best_idx,
                                             int32_t* point_best_dist, uint8_t* point_reached, int32_t* point_stats, const plvs_fuse_lines* L,
                                             const uint8_t* skip_lines, float th_lines, int32_t* line_best_idx, int32_t* line_best_dist,
                                             uint8_t* line_reached, int32_t* line_stats, int32_t* stats, void* stream) {
  return both_kf(kfs, poses, nullptr, n_kfs, P, skip_points, th_points, point_best_idx, point_best_dist, point_reached, point_stats, L, skip_lines,
                 th_lines, line_best_idx, line_best_dist, line_reached, line_stats, stats, stream);
}

// ---- LoopClosing::SearchAndFuse: the Sim3 overloads.  A NULL pose list is refused here: both_kf and the parts tell the two searches
// apart by it (without key frames no part is made, and there is nothing to tell).
int plvs_hip_orb_loop_fuse_search_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3_poses, int n_kfs,
                                     const plvs_fuse_points* P, const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist,
                                     uint8_t* reached, int32_t* stats, void* stream) {
  PLVS_REQUIRE(sim3_poses || n_kfs <= 0, "null poses");
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_point_part_kf(kfs, nullptr, n_kfs, P, skip, th, best_idx, best_dist, reached, stats, false, &part, sim3_poses);
  return rc != PLVS_OK ? rc : fj::run_single(part.get(), stats, 4, stream, false);
}

int plvs_hip_line_loop_fuse_search_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3_poses, int n_kfs,
                                      const plvs_fuse_lines* L, const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist,
                                      uint8_t* reached, int32_t* stats, void* stream) {
  PLVS_REQUIRE(sim3_poses || n_kfs <= 0, "null poses");
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_line_part_kf(kfs, nullptr, n_kfs, L, skip, th, best_idx, best_dist, reached, stats, false, &part, sim3_poses);
  return rc != PLVS_OK ? rc : fj::run_single(part.get(), stats, 4, stream, false);
}

int plvs_hip_orb_loop_fuse_search_kf_host(const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3_poses, int n_kfs,
                                          const plvs_fuse_points* P, const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist,
                                          uint8_t* reached, int32_t* stats) {
  PLVS_REQUIRE(sim3_poses || n_kfs <= 0, "null poses");
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_point_part_kf(kfs, nullptr, n_kfs, P, skip, th, best_idx, best_dist, reached, stats, true, &part, sim3_poses);
  return rc != PLVS_OK ? rc : fj::run_single(part.get(), stats, 4, nullptr, true);
}

int plvs_hip_line_loop_fuse_search_kf_host(const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3_poses, int n_kfs,
                                           const plvs_fuse_lines* L, const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist,
                                           uint8_t* reached, int32_t* stats) {
  PLVS_REQUIRE(sim3_poses || n_kfs <= 0, "null poses");
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_line_part_kf(kfs, nullptr, n_kfs, L, skip, th, best_idx, best_dist, reached, stats, true, &part, sim3_poses);
  return rc != PLVS_OK ? rc : fj::run_single(part.get(), stats, 4, nullptr, true);
}

int plvs_hip_loop_fuse_search_points_and_lines_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3_poses, int n_kfs,
                                                  const plvs_fuse_points* P, const uint8_t* skip_points, float th_points,
                                                  int32_t* point_best_idx, int32_t* point_best_dist, uint8_t* point_reached,
                                                  int32_t* point_stats, const plvs_fuse_lines* L, const uint8_t* skip_lines, float th_lines,
                                                  int32_t* line_best_idx, int32_t* line_best_dist, uint8_t* line_reached, int32_t* line_stats,
                                                  int32_t* stats, void* stream) {
  PLVS_REQUIRE(sim3_poses || n_kfs <= 0, "null poses");
  return both_kf(kfs, nullptr, sim3_poses, n_kfs, P, skip_points, th_points, point_best_idx, point_best_dist, point_reached, point_stats, L,
                 skip_lines, th_lines, line_best_idx, line_best_dist, line_reached, line_stats, stats, stream);
}

}  // extern "C"

// ---- Loop detection: the SearchByProjection(pKF, Scw, ...) overloads (orb_loop_search.hip, line_loop_search.hip).  nmatches of
// a call without pairs (no part is made) is zeroed here, behind every refusal; a part writes its own with its other outputs.
static void zero_nmatches(int32_t* nmatches, int n_kfs) {
  for (int k = 0; nmatches && k < n_kfs; ++k) nmatches[k] = 0;
}

extern "C" {

int plvs_hip_orb_loop_search_by_projection_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3_poses, int n_kfs,
                                              const plvs_fuse_points* P, const uint8_t* skip, const uint8_t* const* occupied, float th,
                                              float ratio_hamming, int projection, int32_t* match_idx, int32_t* match_dist, uint8_t* reached,
                                              int32_t* nmatches, int32_t* stats, void* stream) {
  PLVS_REQUIRE(sim3_poses || n_kfs <= 0, "null poses");
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_loop_search_point_part(kfs, sim3_poses, n_kfs, P, skip, occupied, th, ratio_hamming, projection, match_idx, match_dist,
                                                 reached, nmatches, stats, false, &part);
  if (rc != PLVS_OK) return rc;
  if (!part) zero_nmatches(nmatches, n_kfs);
  return fj::run_single(part.get(), stats, 5, stream, false);
}

int plvs_hip_orb_loop_search_by_projection_kf_host(const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3_poses, int n_kfs,
                                                   const plvs_fuse_points* P, const uint8_t* skip, const uint8_t* const* occupied, float th,
                                                   float ratio_hamming, int projection, int32_t* match_idx, int32_t* match_dist,
                                                   uint8_t* reached, int32_t* nmatches, int32_t* stats) {
  PLVS_REQUIRE(sim3_poses || n_kfs <= 0, "null poses");
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_loop_search_point_part(kfs, sim3_poses, n_kfs, P, skip, occupied, th, ratio_hamming, projection, match_idx, match_dist,
                                                 reached, nmatches, stats, true, &part);
  if (rc != PLVS_OK) return rc;
  if (!part) zero_nmatches(nmatches, n_kfs);
  return fj::run_single(part.get(), stats, 5, nullptr, true);
}

int plvs_hip_line_loop_search_by_projection_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3_poses, int n_kfs,
                                               const plvs_fuse_lines* L, const uint8_t* skip, const uint8_t* const* occupied, float th,
                                               float ratio_hamming, int32_t* match_idx, int32_t* match_dist, uint8_t* reached, int32_t* nmatches,
                                               int32_t* stats, void* stream) {
  PLVS_REQUIRE(sim3_poses || n_kfs <= 0, "null poses");
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_loop_search_line_part(kfs, sim3_poses, n_kfs, L, skip, occupied, th, ratio_hamming, match_idx, match_dist, reached,
                                                nmatches, stats, false, &part);
  if (rc != PLVS_OK) return rc;
  if (!part) zero_nmatches(nmatches, n_kfs);
  return fj::run_single(part.get(), stats, 5, stream, false);
}

int plvs_hip_line_loop_search_by_projection_kf_host(const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3_poses, int n_kfs,
                                                    const plvs_fuse_lines* L, const uint8_t* skip, const uint8_t* const* occupied, float th,
                                                    float ratio_hamming, int32_t* match_idx, int32_t* match_dist, uint8_t* reached,
                                                    int32_t* nmatches, int32_t* stats) {
  PLVS_REQUIRE(sim3_poses || n_kfs <= 0, "null poses");
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_loop_search_line_part(kfs, sim3_poses, n_kfs, L, skip, occupied, th, ratio_hamming, match_idx, match_dist, reached,
                                                nmatches, stats, true, &part);
  if (rc != PLVS_OK) return rc;
  if (!part) zero_nmatches(nmatches, n_kfs);
  return fj::run_single(part.get(), stats, 5, nullptr, true);
}

int plvs_hip_loop_search_by_projection_points_and_lines_kf(
    const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3_poses, int n_kfs, const plvs_fuse_points* P, const uint8_t* skip_points,
    const uint8_t* const* occupied_points, float th_points, float ratio_hamming_points, int projection, int32_t* point_match_idx,
    int32_t* point_match_dist, uint8_t* point_reached, int32_t* point_nmatches, int32_t* point_stats, const plvs_fuse_lines* L,
    const uint8_t* skip_lines, const uint8_t* const* occupied_lines, float th_lines, float ratio_hamming_lines, int32_t* line_match_idx,
    int32_t* line_match_dist, uint8_t* line_reached, int32_t* line_nmatches, int32_t* line_stats, int32_t* stats, void* stream) {
  PLVS_REQUIRE(P || L, "neither points nor lines");
  PLVS_REQUIRE(sim3_poses || n_kfs <= 0, "null poses");
  std::unique_ptr<fj::Part> points, lines;
  if (P) {   // both kinds' refusals before anything is launched or written
    const int rc = fj::make_loop_search_point_part(kfs, sim3_poses, n_kfs, P, skip_points, occupied_points, th_points, ratio_hamming_points,
                                                   projection, point_match_idx, point_match_dist, point_reached, point_nmatches, point_stats,
                                                   false, &points);
    if (rc != PLVS_OK) return rc;
  }
  if (L) {
    const int rc = fj::make_loop_search_line_part(kfs, sim3_poses, n_kfs, L, skip_lines, occupied_lines, th_lines, ratio_hamming_lines,
                                                  line_match_idx, line_match_dist, line_reached, line_nmatches, line_stats, false, &lines);
    if (rc != PLVS_OK) return rc;
  }
  for (int s = 0; s < 5; ++s) {
    if (P && point_stats) point_stats[s] = 0;
    if (L && line_stats) line_stats[s] = 0;
  }
  if (P && !points) zero_nmatches(point_nmatches, n_kfs);
  if (L && !lines) zero_nmatches(line_nmatches, n_kfs);
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  int launches = 0, waits = 0;
  size_t copied = 0;
  const int rc = fj::run_parts(points.get(), lines.get(), static_cast<hipStream_t>(stream), stream == nullptr, false, &launches, &waits, &copied);
  if (stats) { stats[0] = launches; stats[1] = waits; stats[2] = (int32_t)copied; }
  return rc;
}

}  // extern "C"

// ---- SearchByBoW over handles (orb_bow_search.hip): one key frame against K key frames, and K key frames against one frame
static int bow_search(const plvs_keyframe* kf1, const uint8_t* valid1, const plvs_keyframe* const* kfs, const uint8_t* const* valid, int n_kfs,
                      const plvs_bow_frame* F, bool frame_kind, float nn_ratio, int check_orientation, int32_t* match, int32_t* match_dist,
                      int32_t* nmatches, int32_t* stats, void* stream, bool host_entry) {
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_bow_search_part(kf1, valid1, kfs, valid, n_kfs, F, frame_kind, nn_ratio, check_orientation, match, match_dist,
                                          nmatches, stats, host_entry, &part);
  return rc != PLVS_OK ? rc : fj::run_single(part.get(), stats, 6, stream, host_entry);
}

extern "C" {

int plvs_hip_orb_search_by_bow_kf(const plvs_keyframe* kf1, const uint8_t* valid1, const plvs_keyframe* const* kfs2,
                                  const uint8_t* const* valid2, int n_kfs2, float nn_ratio, int check_orientation, int32_t* match_idx,
                                  int32_t* match_dist, int32_t* nmatches, int32_t* stats, void* stream) {
  return bow_search(kf1, valid1, kfs2, valid2, n_kfs2, nullptr, false, nn_ratio, check_orientation, match_idx, match_dist, nmatches, stats,
                    stream, false);
}

int plvs_hip_orb_search_by_bow_frame_kf(const plvs_keyframe* const* kfs, const uint8_t* const* kf_valid, int n_kfs, const plvs_bow_frame* F,
                                        float nn_ratio, int check_orientation, int32_t* assigned, int32_t* match_dist, int32_t* nmatches,
                                        int32_t* stats, void* stream) {
  return bow_search(nullptr, nullptr, kfs, kf_valid, n_kfs, F, true, nn_ratio, check_orientation, assigned, match_dist, nmatches, stats, stream,
                    false);
}

int plvs_hip_orb_search_by_bow_kf_host(const plvs_keyframe* kf1, const uint8_t* valid1, const plvs_keyframe* const* kfs2,
                                       const uint8_t* const* valid2, int n_kfs2, float nn_ratio, int check_orientation, int32_t* match_idx,
                                       int32_t* match_dist, int32_t* nmatches, int32_t* stats) {
  return bow_search(kf1, valid1, kfs2, valid2, n_kfs2, nullptr, false, nn_ratio, check_orientation, match_idx, match_dist, nmatches, stats,
                    nullptr, true);
}

int plvs_hip_orb_search_by_bow_frame_kf_host(const plvs_keyframe* const* kfs, const uint8_t* const* kf_valid, int n_kfs,
                                             const plvs_bow_frame* F, float nn_ratio, int check_orientation, int32_t* assigned,
                                             int32_t* match_dist, int32_t* nmatches, int32_t* stats) {
  return bow_search(nullptr, nullptr, kfs, kf_valid, n_kfs, F, true, nn_ratio, check_orientation, assigned, match_dist, nmatches, stats, nullptr,
                    true);
}

}  // extern "C"
