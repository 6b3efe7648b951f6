// ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints)
// (reference src/ORBmatcher.cc:71-244) and SearchByProjection(CurrentFrame, LastFrame, th, bMono)
// (:1774-1993) for monocular / RGB-D frames, replaced at the
// search-function level: the Hamming distances of every (map point, candidate
// keypoint) pair are computed in one batched launch; the parts that are sequential by
// definition — the candidate windows on the 64x48 frame grid (Frame::GetFeaturesInArea,
// src/Frame.cc:1231-1303) and the greedy best / second-best assignment, in which a keypoint
// claimed by an earlier map point is skipped by the later ones — stay on the host, in the
// reference's order.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "orb_window.hpp"

using namespace plvs::orbwin;

constexpr size_t kDirectReadBytes = 96 * 1024;   // inputs up to this size are read in place from pinned host memory

// The pair distances of plvs_hip_hamming_pairs in two steps, for a caller that knows the descriptor sets before it knows
// the pairs (SearchByBoW enumerates them node by node): begin() stages the descriptors and starts their copy, the host
// enumerates, finish() sends the pair lists behind them, launches and waits.  max_pairs bounds the pairs of finish().
struct PairsJob {
  size_t o_pq = 0, o_pt = 0, o_d = 0;
  int nq = 0, nt = 0, max_pairs = 0;
};
int pairs_begin(PairsJob& J, const uint8_t* query, int nq, const uint8_t* train, int nt, int max_pairs) {
  using plvs::up16;
  const size_t o_q = 0, o_t = o_q + up16((size_t)nq * 32);
  J.o_pq = o_t + up16((size_t)nt * 32);
  J.o_pt = J.o_pq + up16(sizeof(int32_t) * (size_t)max_pairs);
  J.o_d = J.o_pt + up16(sizeof(int32_t) * (size_t)max_pairs);
  J.nq = nq; J.nt = nt; J.max_pairs = max_pairs;
  plvs::HostStage& st = plvs::thread_stage();
  PLVS_HIP_TRY(st.reserve(J.o_d + up16(sizeof(int32_t) * (size_t)max_pairs)));
  memcpy(st.pinned + o_q, query, (size_t)nq * 32);
  memcpy(st.pinned + o_t, train, (size_t)nt * 32);
  PLVS_HIP_TRY(hipMemcpyAsync(st.dev, st.pinned, J.o_pq, hipMemcpyHostToDevice, st.stream));
  return PLVS_OK;
}
int pairs_finish(PairsJob& J, const int32_t* pair_q, const int32_t* pair_t, int npairs, int32_t* dist) {
  plvs::HostStage& st = plvs::thread_stage();
  if (npairs == 0) {
    PLVS_HIP_TRY(hipStreamSynchronize(st.stream));
    return PLVS_OK;
  }
  PLVS_REQUIRE(npairs <= J.max_pairs, "more pairs than announced");
  memcpy(st.pinned + J.o_pq, pair_q, sizeof(int32_t) * (size_t)npairs);
  memcpy(st.pinned + J.o_pt, pair_t, sizeof(int32_t) * (size_t)npairs);
  // (the two lists lie apart — max_pairs each —: one copy over both when they are nearly full, two otherwise)
  if ((size_t)npairs * 2 >= (size_t)J.max_pairs) {
    PLVS_HIP_TRY(hipMemcpyAsync(st.dev + J.o_pq, st.pinned + J.o_pq, (J.o_pt - J.o_pq) + sizeof(int32_t) * (size_t)npairs, hipMemcpyHostToDevice, st.stream));
  } else {
    PLVS_HIP_TRY(hipMemcpyAsync(st.dev + J.o_pq, st.pinned + J.o_pq, sizeof(int32_t) * (size_t)npairs, hipMemcpyHostToDevice, st.stream));
    PLVS_HIP_TRY(hipMemcpyAsync(st.dev + J.o_pt, st.pinned + J.o_pt, sizeof(int32_t) * (size_t)npairs, hipMemcpyHostToDevice, st.stream));
  }
  hipLaunchKernelGGL(hamming_pairs_kernel, dim3(plvs::ceil_div(npairs, 256)), dim3(256), 0, st.stream,
                     reinterpret_cast<const uint4*>(st.dev), reinterpret_cast<const uint4*>(st.dev + ((size_t)J.nq * 32 + 15) / 16 * 16),
                     reinterpret_cast<const int32_t*>(st.dev + J.o_pq), reinterpret_cast<const int32_t*>(st.dev + J.o_pt), npairs,
                     reinterpret_cast<int32_t*>(st.pinned + J.o_d));
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(hipStreamSynchronize(st.stream));
  memcpy(dist, st.pinned + J.o_d, sizeof(int32_t) * (size_t)npairs);
  return PLVS_OK;
}

extern "C" {

int plvs_hip_hamming_pairs(const uint8_t* query, int nq, const uint8_t* train, int nt, const int32_t* pair_q,
                           const int32_t* pair_t, int npairs, int32_t* dist) {
  PLVS_REQUIRE(nq >= 0 && nt >= 0 && npairs >= 0, "negative size");
  if (npairs == 0) return PLVS_OK;
  PLVS_REQUIRE(query && train && pair_q && pair_t && dist, "null argument");
  for (int p = 0; p < npairs; ++p)
    PLVS_REQUIRE(pair_q[p] >= 0 && pair_q[p] < nq && pair_t[p] >= 0 && pair_t[p] < nt, "pair index out of range");
  // one staged block: [query | train | pair_q | pair_t] in, [dist] out
  using plvs::up16;
  const size_t o_q = 0, o_t = o_q + up16((size_t)nq * 32), o_pq = o_t + up16((size_t)nt * 32),
               o_pt = o_pq + up16(sizeof(int32_t) * (size_t)npairs), o_d = o_pt + up16(sizeof(int32_t) * (size_t)npairs),
               total = o_d + up16(sizeof(int32_t) * (size_t)npairs);
  plvs::HostStage& st = plvs::thread_stage();
  PLVS_HIP_TRY(st.reserve(total));
  memcpy(st.pinned + o_q, query, (size_t)nq * 32);
  memcpy(st.pinned + o_t, train, (size_t)nt * 32);
  memcpy(st.pinned + o_pq, pair_q, sizeof(int32_t) * (size_t)npairs);
  memcpy(st.pinned + o_pt, pair_t, sizeof(int32_t) * (size_t)npairs);
  // The distances go straight into the pinned block (posted writes over the link); a small call — the line searches: a few
  // hundred descriptors, a thousand pairs — reads its inputs from there as well: one launch and one wait instead of a copy
  // in, a launch, a copy back and a wait (60 us for 5 us of arithmetic).
  const bool direct = o_d <= kDirectReadBytes;   // (measured: 6 us saved at 26 KB, 6 us lost at 230 KB)
  char* const in = direct ? st.pinned : st.dev;
  if (!direct) PLVS_HIP_TRY(hipMemcpyAsync(st.dev, st.pinned, o_d, hipMemcpyHostToDevice, st.stream));
  hipLaunchKernelGGL(hamming_pairs_kernel, dim3(plvs::ceil_div(npairs, 256)), dim3(256), 0, st.stream,
                     reinterpret_cast<const uint4*>(in + o_q), reinterpret_cast<const uint4*>(in + o_t),
                     reinterpret_cast<const int32_t*>(in + o_pq), reinterpret_cast<const int32_t*>(in + o_pt), npairs,
                     reinterpret_cast<int32_t*>(st.pinned + o_d));
  PLVS_KERNEL_CHECK();
  PLVS_HIP_TRY(hipStreamSynchronize(st.stream));   // (spinning on hipStreamQuery instead: no difference, measured)
  memcpy(dist, st.pinned + o_d, sizeof(int32_t) * (size_t)npairs);
  return PLVS_OK;
}

int plvs_hip_orb_search_by_projection(const plvs_frame_view* F, const plvs_mappoint_view* M, float th,
                                      int far_points, float th_far, float nn_ratio, const uint8_t* occupied,
                                      int32_t* assigned, int* nmatches) {
  PLVS_REQUIRE(F && M && assigned && nmatches, "null argument");
  PLVS_REQUIRE(F->n >= 0 && M->m >= 0, "negative size");
  *nmatches = 0;
  for (int i = 0; i < F->n; ++i) assigned[i] = -1;
  if (F->n == 0 || M->m == 0) return PLVS_OK;
  PLVS_REQUIRE(F->x && F->y && F->octave && F->u_right && F->desc && F->scale_factors, "null frame array");
  PLVS_REQUIRE(M->track_in_view && M->bad && M->proj_x && M->proj_y && M->proj_xr && M->view_cos &&
                   M->track_depth && M->level && M->desc,
               "null map-point array");
  const FrameGrid grid(F);
  // ---- candidate windows (GetFeaturesInArea) of every map point the reference would process,
  // in the reference's order; everything but the "already claimed" test is decided here
  std::vector<WinQuery> wq;
  wq.reserve((size_t)M->m);
  const int factor = th != 1.0f ? 1 : 0;
  for (int k = 0; k < M->m; ++k) {
    if (!M->track_in_view[k]) continue;
    if (far_points && M->track_depth[k] > th_far) continue;
    if (M->bad[k]) continue;
    const int level = M->level[k];
    PLVS_REQUIRE(level >= 0, "negative predicted level");
    // a keypoint with a stereo coordinate must agree with the point's predicted one within the radius (RGB-D / stereo frames)
    wq.push_back(map_point_query(M->proj_x[k], M->proj_y[k], M->proj_xr[k], M->view_cos[k], level, th, factor, F->scale_factors[level], k));
  }
  std::vector<int32_t> pair_t, dist, q_at, q_n, src(wq.size());
  int rc = window_candidates(F, grid, wq, M->desc, M->m, q_at, q_n, pair_t, dist);
  if (rc != PLVS_OK) return rc;
  for (size_t k = 0; k < wq.size(); ++k) src[k] = wq[k].src;
  // ---- greedy assignment in map-point order (:106-163)
  const int n = greedy_points(F, src.data(), wq.size(), q_at, q_n, pair_t, dist, nn_ratio, occupied, M->has_obs, assigned);
  *nmatches = n;
  return PLVS_OK;
}

int plvs_hip_orb_search_by_projection_ff(const plvs_frame_view* F, const float* cur_angle, float max_x, float max_y,
                                         float mbf, const plvs_lastframe_view* L, float th, int forward,
                                         int backward, int check_orientation, const uint8_t* occupied,
                                         int32_t* assigned, int* nmatches) {
  PLVS_REQUIRE(F && L && assigned && nmatches, "null argument");
  PLVS_REQUIRE(F->n >= 0 && L->n >= 0, "negative size");
  *nmatches = 0;
  for (int i = 0; i < F->n; ++i) assigned[i] = -1;
  if (F->n == 0 || L->n == 0) return PLVS_OK;
  PLVS_REQUIRE(F->x && F->y && F->octave && F->u_right && F->desc && F->scale_factors && cur_angle,
               "null frame array");
  PLVS_REQUIRE(L->valid && L->u && L->v && L->invz && L->octave && L->angle && L->desc, "null last-frame array");
  const FrameGrid grid(F);
  // ---- the queries the reference would run (:1800-1840), then their windows and distances on the device
  std::vector<WinQuery> wq;
  wq.reserve((size_t)L->n);
  for (int i = 0; i < L->n; ++i) {
    if (!L->valid[i]) continue;
    const float invzc = L->invz[i];
    if (invzc < 0) continue;
    const float u = L->u[i], v = L->v[i];
    if (u < F->min_x || u > max_x) continue;
    if (v < F->min_y || v > max_y) continue;
    const int oct = L->octave[i];
    PLVS_REQUIRE(oct >= 0, "negative octave");
    wq.push_back(last_frame_query(u, v, invzc, oct, th, F->scale_factors[oct], mbf, forward, backward, i));
  }
  std::vector<int32_t> pair_t, dist, q_at, q_n, src(wq.size());
  int rc = window_candidates(F, grid, wq, L->desc, L->n, q_at, q_n, pair_t, dist);
  if (rc != PLVS_OK) return rc;
  for (size_t k = 0; k < wq.size(); ++k) src[k] = wq[k].src;
  *nmatches = greedy_last_frame_points(F, cur_angle, src.data(), wq.size(), q_at, q_n, pair_t, dist, L->angle, L->has_obs, check_orientation,
                                       occupied, assigned);
  return PLVS_OK;
}

int plvs_hip_orb_search_by_bow(const plvs_featvec_view* KV, const uint8_t* kf_desc, int kf_n,
                               const uint8_t* kf_valid, const float* kf_angle, const plvs_featvec_view* FV,
                               const uint8_t* f_desc, int f_n, const float* f_angle, float nn_ratio,
                               int check_orientation, int32_t* assigned, int* nmatches) {
  PLVS_REQUIRE(KV && FV && nmatches, "null argument");
  PLVS_REQUIRE(kf_n >= 0 && f_n >= 0 && KV->nnodes >= 0 && FV->nnodes >= 0, "negative size");
  PLVS_REQUIRE(f_n == 0 || assigned, "assigned is null");
  *nmatches = 0;
  for (int i = 0; i < f_n; ++i) assigned[i] = -1;
  if (kf_n == 0 || f_n == 0 || KV->nnodes == 0 || FV->nnodes == 0) return PLVS_OK;
  PLVS_REQUIRE(KV->node_id && KV->offset && KV->index && FV->node_id && FV->offset && FV->index,
               "null feature-vector array");
  PLVS_REQUIRE(kf_desc && kf_valid && f_desc, "null descriptor / validity array");
  PLVS_REQUIRE(!check_orientation || (kf_angle && f_angle), "angles needed for the orientation check");
  for (int a = 0; a < KV->nnodes; ++a) {
    PLVS_REQUIRE(KV->offset[a] <= KV->offset[a + 1], "key-frame offsets not monotone");
    PLVS_REQUIRE(a == 0 || KV->node_id[a - 1] < KV->node_id[a], "key-frame node ids must ascend (std::map order)");
  }
  for (int b = 0; b < FV->nnodes; ++b) {
    PLVS_REQUIRE(FV->offset[b] <= FV->offset[b + 1], "frame offsets not monotone");
    PLVS_REQUIRE(b == 0 || FV->node_id[b - 1] < FV->node_id[b], "frame node ids must ascend (std::map order)");
  }
  for (int k = KV->offset[0]; k < KV->offset[KV->nnodes]; ++k)
    PLVS_REQUIRE(KV->index[k] < (uint32_t)kf_n, "key-frame feature index out of range");
  for (int k = FV->offset[0]; k < FV->offset[FV->nnodes]; ++k)
    PLVS_REQUIRE(FV->index[k] < (uint32_t)f_n, "frame feature index out of range");

  // Every (key-frame feature, frame feature) pair of every common vocabulary node, in the
  // reference's visiting order; one launch for all distances, then the greedy pass on the host.
  struct Query { int kf; int first, count; };
  std::vector<Query> queries;
  std::vector<int32_t> pair_q, pair_t;
  // the descriptors are on their way to the device while the pairs are enumerated (a walk over the nodes alone bounds them)
  PairsJob job;
  plvs::StreamGuard guard;   // (an error return between begin and finish must not leave the copy in flight on the staging block)
  {
    long long bound = 0;
    int a0 = 0, b0 = 0;
    while (a0 < KV->nnodes && b0 < FV->nnodes) {
      if (KV->node_id[a0] == FV->node_id[b0]) {
        bound += (long long)(KV->offset[a0 + 1] - KV->offset[a0]) * (FV->offset[b0 + 1] - FV->offset[b0]);
        ++a0; ++b0;
      } else if (KV->node_id[a0] < FV->node_id[b0]) ++a0;
      else ++b0;
    }
    PLVS_REQUIRE(bound < (1ll << 30), "too many candidate pairs");
    if (bound == 0) return PLVS_OK;
    const int rcb = pairs_begin(job, kf_desc, kf_n, f_desc, f_n, (int)bound);
    if (rcb != PLVS_OK) return rcb;
    guard.s = plvs::thread_stage().stream;
    guard.armed = true;
    pair_q.reserve((size_t)bound);
    pair_t.reserve((size_t)bound);
  }
  int a = 0, b = 0;
  while (a < KV->nnodes && b < FV->nnodes) {   // the lower_bound walk of :327-489
    if (KV->node_id[a] == FV->node_id[b]) {
      for (int ik = KV->offset[a]; ik < KV->offset[a + 1]; ++ik) {
        const int real_kf = (int)KV->index[ik];
        if (!kf_valid[real_kf]) continue;   // !pMP || pMP->isBad()
        Query q{real_kf, (int)pair_q.size(), FV->offset[b + 1] - FV->offset[b]};
        for (int jf = FV->offset[b]; jf < FV->offset[b + 1]; ++jf) {
          pair_q.push_back(real_kf);
          pair_t.push_back((int32_t)FV->index[jf]);
        }
        if (q.count) queries.push_back(q);
      }
      ++a;
      ++b;
    } else if (KV->node_id[a] < FV->node_id[b]) {
      ++a;
    } else {
      ++b;
    }
  }
  std::vector<int32_t> dist(pair_q.size());
  int rc = pairs_finish(job, pair_q.data(), pair_t.data(), (int)pair_q.size(), dist.data());
  guard.armed = false;
  if (rc != PLVS_OK) return rc;
  std::vector<int> hist_item, hist_bin;
  const float factor = kHistoLength / 360.0f;   // USE_NEW_HISTOGRAM_FACTOR, :52, :313
  int n = 0;
  for (const Query& q : queries) {
    int best1 = 256, best_idx = -1, best2 = 256;
    for (int p = q.first; p < q.first + q.count; ++p) {
      const int i_f = pair_t[p];
      if (assigned[i_f] >= 0) continue;   // vpMapPointMatches[realIdxF]
      const int d = dist[p];
      if (d < best1) {
        best2 = best1;
        best1 = d;
        best_idx = i_f;
      } else if (d < best2) {
        best2 = d;
      }
    }
    if (best1 <= kThLow && (float)best1 < nn_ratio * (float)best2) {
      assigned[best_idx] = q.kf;
      ++n;
      if (check_orientation) {
        float rot = kf_angle[q.kf] - f_angle[best_idx];
        if (rot < 0.0) rot += 360.0f;
        int bin = (int)std::round(rot * factor);
        if (bin == kHistoLength) bin = 0;
        hist_item.push_back(best_idx);
        hist_bin.push_back(bin);
      }
    }
  }
  if (check_orientation) {
    int count[kHistoLength] = {0};
    for (int bn : hist_bin) ++count[bn];
    int ind1, ind2, ind3;
    three_maxima(count, kHistoLength, ind1, ind2, ind3);
    for (size_t k = 0; k < hist_bin.size(); ++k)
      if (hist_bin[k] != ind1 && hist_bin[k] != ind2 && hist_bin[k] != ind3) {
        assigned[hist_item[k]] = -1;
        --n;
      }
  }
  *nmatches = n;
  return PLVS_OK;
}

}  // extern "C"
