// The candidate windows of the point searches — Frame::AssignFeaturesToGrid / GetFeaturesInArea as a CSR grid, the window
// kernel that walks it, that kernel's one staging (WindowStage) and its launch as a call of its own (window_candidates) — and the
// greedy passes of SearchByProjection(F, MapPoints) and SearchByProjection(CurrentFrame, LastFrame): what the two entries of
// orb_search.hip do once their inputs exist, shared with the one-call searches (frame_track.hip, frame_motion.hip), whose projection
// kernels write the queries the stage's launch reads.  Everything sits in an unnamed namespace: each translation unit that includes
// this gets its own copy.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"

namespace plvs {
namespace orbwin {
namespace {

constexpr int kGridCols = 64;   // FRAME_GRID_COLS, include/Frame.h:68
constexpr int kGridRows = 48;   // FRAME_GRID_ROWS, include/Frame.h:67
constexpr int kThHigh = 100;    // ORBmatcher::TH_HIGH, src/ORBmatcher.cc:57
constexpr int kThLow = 50;      // ORBmatcher::TH_LOW, :58
constexpr int kHistoLength = 12; // ORBmatcher::HISTO_LENGTH, :61

// dist[p] = ORBmatcher::DescriptorDistance(query[pair_q[p]], train[pair_t[p]]) (src/ORBmatcher.cc:2198)
__global__ __launch_bounds__(256) void hamming_pairs_kernel(const uint4* __restrict__ query,
                                                            const uint4* __restrict__ train,
                                                            const int32_t* __restrict__ pair_q,
                                                            const int32_t* __restrict__ pair_t, int npairs,
                                                            int32_t* __restrict__ dist) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npairs) return;
  const uint4 a0 = query[2 * pair_q[p]], a1 = query[2 * pair_q[p] + 1];
  const uint4 b0 = train[2 * pair_t[p]], b1 = train[2 * pair_t[p] + 1];
  dist[p] = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
            __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// Frame::AssignFeaturesToGrid (src/Frame.cc:717-752): cell lists in keypoint order
struct FrameGrid {
  // mGrid as one array in the reference's enumeration order — column ix, row iy, insertion order inside the cell —
  // with the fields the window test reads next to the index: a window is one contiguous range per column.
  struct Member { float x, y; int octave, idx; };
  std::vector<int> start;
  std::vector<Member> members;
  explicit FrameGrid(const plvs_frame_view* F) : start(kGridCols * kGridRows + 1, 0), members(F->n) {
    std::vector<int> cell(F->n);
    for (int i = 0; i < F->n; ++i) {
      const int px = (int)std::round((F->x[i] - F->min_x) * F->grid_w_inv);   // PosInGrid, :1305-1316
      const int py = (int)std::round((F->y[i] - F->min_y) * F->grid_h_inv);
      cell[i] = (px < 0 || px >= kGridCols || py < 0 || py >= kGridRows) ? -1 : px * kGridRows + py;
      if (cell[i] >= 0) ++start[cell[i] + 1];
    }
    for (int c = 0; c < kGridCols * kGridRows; ++c) start[c + 1] += start[c];
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int i = 0; i < F->n; ++i)
      if (cell[i] >= 0) members[fill[cell[i]]++] = Member{F->x[i], F->y[i], F->octave[i], i};
  }
  // Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) (src/Frame.cc:1231-1303), appended to `out`
  // in the reference's order (defaults: minLevel = -1, maxLevel = kMaxInt, include/Frame.h:173)
  template <typename Fn>
  void for_each_in_area(const plvs_frame_view* F, float x, float y, float r, int min_level, int max_level, Fn&& fn) const {
    int c0 = (int)std::floor((x - F->min_x - r) * F->grid_w_inv);
    if (c0 < 0) c0 = 0;
    if (c0 >= kGridCols) return;
    int c1 = (int)std::ceil((x - F->min_x + r) * F->grid_w_inv);
    if (c1 > kGridCols - 1) c1 = kGridCols - 1;
    if (c1 < 0) return;
    int r0 = (int)std::floor((y - F->min_y - r) * F->grid_h_inv);
    if (r0 < 0) r0 = 0;
    if (r0 >= kGridRows) return;
    int r1 = (int)std::ceil((y - F->min_y + r) * F->grid_h_inv);
    if (r1 > kGridRows - 1) r1 = kGridRows - 1;
    if (r1 < 0) return;
    const bool check_levels = (min_level > 0) || (max_level >= 0);
    for (int ix = c0; ix <= c1; ++ix) {
      const Member* m = members.data() + start[ix * kGridRows + r0];
      const Member* const end = members.data() + start[ix * kGridRows + r1 + 1];   // rows r0 .. r1 of the column
      for (; m < end; ++m) {
        if (check_levels && (m->octave < min_level || m->octave > max_level)) continue;
        const float dx = m->x - x, dy = m->y - y;
        if (std::fabs(dx) < r && std::fabs(dy) < r) fn(m->idx);
      }
    }
  }
};

// Frame::GetFeaturesInArea + the stereo gate + the Hamming distance of every candidate, on the device: a wave per
// query walks the query's grid window in the reference's order — column after column, each column's rows one
// contiguous range of the CSR members —, and the accepted candidates leave as (index, distance) in that order (ballot
// compaction keeps it).  Two passes over the window: count, reserve the query's output range, emit.
struct WinQuery {
  float u, v, r, ur;            // window centre, radius, predicted right coordinate
  int min_level, max_level;     // inclusive; tested only when check_levels
  int src;                      // descriptor row of the query
  int check_levels;
};
struct WinFrame {
  const FrameGrid::Member* members;
  const int* start;
  const float* u_right;
  const uint4* desc;            // two uint4 per keypoint
  float min_x, min_y, grid_w_inv, grid_h_inv;
};
__global__ __launch_bounds__(256) void orb_window_candidates(const WinQuery* __restrict__ queries, int nq, WinFrame F,
                                                             const uint4* __restrict__ qdesc, uint32_t* __restrict__ cursor,
                                                             int32_t* __restrict__ q_first, int32_t* __restrict__ q_count,
                                                             int2* __restrict__ out, uint32_t out_cap) {
  const int lane = threadIdx.x & 63;
  const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qi >= nq) return;
  const WinQuery q = queries[qi];
  int c0 = (int)floorf((q.u - F.min_x - q.r) * F.grid_w_inv);
  int c1 = (int)ceilf((q.u - F.min_x + q.r) * F.grid_w_inv);
  int r0 = (int)floorf((q.v - F.min_y - q.r) * F.grid_h_inv);
  int r1 = (int)ceilf((q.v - F.min_y + q.r) * F.grid_h_inv);
  bool empty = c0 >= kGridCols || c1 < 0 || r0 >= kGridRows || r1 < 0 || !(q.r >= 0.0f);   // (a negative radius accepts nothing)
  c0 = max(c0, 0); c1 = min(c1, kGridCols - 1); r0 = max(r0, 0); r1 = min(r1, kGridRows - 1);
  auto accept = [&](const FrameGrid::Member& m) {
    if (q.check_levels && (m.octave < q.min_level || m.octave > q.max_level)) return false;
    const float dx = m.x - q.u, dy = m.y - q.v;
    if (!(fabsf(dx) < q.r && fabsf(dy) < q.r)) return false;
    const float ur = F.u_right[m.idx];
    if (ur > 0) {
      const float er = fabsf(q.ur - ur);
      if (er > q.r) return false;
    }
    return true;
  };
  uint32_t total = 0;
  if (!empty)
    for (int ix = c0; ix <= c1; ++ix) {
      const int s = F.start[ix * kGridRows + r0], e = F.start[ix * kGridRows + r1 + 1];
      for (int b = s; b < e; b += 64) {
        const bool ok = b + lane < e && accept(F.members[b + lane]);
        total += (uint32_t)__popcll(__ballot(ok));
      }
    }
  uint32_t first = 0;
  if (lane == 0) {
    first = total ? atomicAdd(cursor, total) : 0u;
    q_first[qi] = (int32_t)first;
    q_count[qi] = (int32_t)total;
  }
  first = (uint32_t)__shfl((int)first, 0);
  if (total == 0 || first + total > out_cap) return;   // (the host sees cursor > out_cap and repeats with more room)
  const uint4 qa = qdesc[2 * (size_t)q.src], qb = qdesc[2 * (size_t)q.src + 1];
  uint32_t at = first;
  for (int ix = c0; ix <= c1; ++ix) {
    const int s = F.start[ix * kGridRows + r0], e = F.start[ix * kGridRows + r1 + 1];
    for (int b = s; b < e; b += 64) {
      FrameGrid::Member m{};
      bool ok = false;
      if (b + lane < e) {
        m = F.members[b + lane];
        ok = accept(m);
      }
      const unsigned long long mask = __ballot(ok);
      if (ok) {
        const uint4 ta = F.desc[2 * (size_t)m.idx], tb = F.desc[2 * (size_t)m.idx + 1];
        const int d = __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                      __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
        out[at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = make_int2(m.idx, d);
      }
      at += (uint32_t)__popcll(mask);
    }
  }
}

// One orb_window_candidates launch over frame F with nq queries, as a share of a staging block (a fusejob::Part in small): it
// takes its places through the caller's allocator — inputs the caller copies in one piece, scratch that lives in HBM only, outputs
// the kernel posts into the pinned side —, fills its inputs, launches, and after the caller's wait unpacks.  The queries are either
// host-built (host_wq: they travel inside the input share) or written at queries(dev) by an earlier kernel on the same stream.
struct WindowStage {
  const plvs_frame_view* F = nullptr;
  const FrameGrid* grid = nullptr;
  int nq = 0, n_qdesc = 0;             // nq == 0: a stage that takes nothing and is not launched
  const uint8_t* qdesc = nullptr;      // the queries' descriptor rows (n_qdesc x 32)
  const WinQuery* host_wq = nullptr;
  size_t out_cap = 0;                  // before take_outputs: a caller that knows the count already; after: the records there is room for
  size_t o_wq = 0, o_mem = 0, o_start = 0, o_ur = 0, o_fd = 0, o_qd = 0, o_cur = 0, o_first = 0, o_count = 0, o_rec = 0;

  void take_inputs(plvs::Take& take) {
    if (nq == 0) return;
    if (host_wq) o_wq = take(sizeof(WinQuery) * (size_t)nq);
    o_mem = take(sizeof(FrameGrid::Member) * grid->members.size()); o_start = take(sizeof(int) * grid->start.size());
    o_ur = take(sizeof(float) * (size_t)F->n); o_fd = take((size_t)F->n * 32); o_qd = take((size_t)n_qdesc * 32);
    o_cur = take(16);   // (stays in HBM: it is the target of the waves' atomics)
  }
  void take_scratch(plvs::Take& take) { if (nq && !host_wq) o_wq = take(sizeof(WinQuery) * (size_t)nq); }
  // (first / count / records go straight into the pinned block — posted writes over the link, a few tens of KB —: one copy in, one
  // launch, one wait; the copies back and the second wait they needed cost more than the search's arithmetic)
  void take_outputs(plvs::Take& take) {
    if (nq == 0) return;
    out_cap = std::max((size_t)nq * 32 + 4096, out_cap);
    o_first = take(sizeof(int32_t) * (size_t)nq); o_count = take(sizeof(int32_t) * (size_t)nq);
    o_rec = take(sizeof(int2) * out_cap);
  }
  void fill(char* pinned) const {
    if (nq == 0) return;
    if (host_wq) memcpy(pinned + o_wq, host_wq, sizeof(WinQuery) * (size_t)nq);
    memcpy(pinned + o_mem, grid->members.data(), sizeof(FrameGrid::Member) * grid->members.size());
    memcpy(pinned + o_start, grid->start.data(), sizeof(int) * grid->start.size());
    memcpy(pinned + o_ur, F->u_right, sizeof(float) * (size_t)F->n);
    memcpy(pinned + o_fd, F->desc, (size_t)F->n * 32);
    memcpy(pinned + o_qd, qdesc, (size_t)n_qdesc * 32);
    memset(pinned + o_cur, 0, 16);
  }
  WinQuery* queries(char* dev) const { return reinterpret_cast<WinQuery*>(dev + o_wq); }
  int launch(char* dev, char* pinned, hipStream_t stream) const {
    if (nq == 0) return PLVS_OK;
    const WinFrame wf{reinterpret_cast<const FrameGrid::Member*>(dev + o_mem), reinterpret_cast<const int*>(dev + o_start),
                      reinterpret_cast<const float*>(dev + o_ur), reinterpret_cast<const uint4*>(dev + o_fd),
                      F->min_x, F->min_y, F->grid_w_inv, F->grid_h_inv};
    hipLaunchKernelGGL(orb_window_candidates, dim3(plvs::ceil_div((size_t)nq, 4)), dim3(256), 0, stream, queries(dev), nq, wf,
                       reinterpret_cast<const uint4*>(dev + o_qd), reinterpret_cast<uint32_t*>(dev + o_cur),
                       reinterpret_cast<int32_t*>(pinned + o_first), reinterpret_cast<int32_t*>(pinned + o_count),
                       reinterpret_cast<int2*>(pinned + o_rec), (uint32_t)out_cap);
    PLVS_KERNEL_CHECK();
    return PLVS_OK;
  }
  // After the wait: *found candidates in all; false when they are more than the block had room for (a spill: nothing is written),
  // else per query k its candidates pair_t / dist [q_at[k], q_at[k] + q_n[k]) in the reference's enumeration order.
  bool unpack(const char* pinned, size_t* found, std::vector<int32_t>& q_at, std::vector<int32_t>& q_n, std::vector<int32_t>& pair_t,
              std::vector<int32_t>& dist) const {
    const int32_t* qf = reinterpret_cast<const int32_t*>(pinned + o_first);
    const int32_t* qc = reinterpret_cast<const int32_t*>(pinned + o_count);
    *found = 0;
    for (int k = 0; k < nq; ++k) *found += (size_t)qc[k];
    if (*found > out_cap) return false;
    const int2* rec = reinterpret_cast<const int2*>(pinned + o_rec);
    pair_t.resize(*found);
    dist.resize(*found);
    // (the ranges were reserved in the order the waves arrived: copied here query after query)
    uint32_t at = 0;
    for (int k = 0; k < nq; ++k) {
      q_at[k] = (int32_t)at;
      q_n[k] = qc[k];
      for (int c = 0; c < qc[k]; ++c) { pair_t[at + c] = rec[qf[k] + c].x; dist[at + c] = rec[qf[k] + c].y; }
      at += (uint32_t)qc[k];
    }
    return true;
  }
};

// The windows of `wq` on frame F as a call of its own, on the thread's own stream and staging block: per query k the accepted
// candidates pair_t / dist [q_at[k], q_at[k] + q_n[k]).  One repetition with the room that is needed when the first launch spills.
int window_candidates(const plvs_frame_view* F, const FrameGrid& grid, const std::vector<WinQuery>& wq, const uint8_t* qdesc,
                      int n_qdesc, std::vector<int32_t>& q_at, std::vector<int32_t>& q_n, std::vector<int32_t>& pair_t,
                      std::vector<int32_t>& dist, size_t first_cap = 0, int* launches = nullptr) {
  const int nq = (int)wq.size();
  q_at.assign((size_t)nq, 0);
  q_n.assign((size_t)nq, 0);
  pair_t.clear();
  dist.clear();
  if (nq == 0) return PLVS_OK;
  plvs::HostStage& st = plvs::thread_stage();
  for (int attempt = 0;; ++attempt) {
    if (launches) ++*launches;
    WindowStage W{F, &grid, nq, n_qdesc, qdesc, wq.data(), first_cap};
    plvs::Take take;
    W.take_inputs(take);
    const size_t in_end = take.at;
    W.take_outputs(take);
    PLVS_HIP_TRY(st.reserve(take.at));
    W.fill(st.pinned);
    PLVS_HIP_TRY(hipMemcpyAsync(st.dev, st.pinned, in_end, hipMemcpyHostToDevice, st.stream));
    const int rc = W.launch(st.dev, st.pinned, st.stream);
    if (rc != PLVS_OK) return rc;
    PLVS_HIP_TRY(hipStreamSynchronize(st.stream));
    size_t found = 0;
    if (W.unpack(st.pinned, &found, q_at, q_n, pair_t, dist)) return PLVS_OK;
    PLVS_REQUIRE(attempt == 0, "candidate count changed between two identical launches");
    first_cap = found + 64;   // more candidates than room: once more with what is needed
  }
}

// ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:2123-2170) on bin counts
void three_maxima(const int* count, int L, int& ind1, int& ind2, int& ind3) {
  int max1 = 0, max2 = 0, max3 = 0;
  ind1 = ind2 = ind3 = -1;
  for (int i = 0; i < L; ++i) {
    const int s = count[i];
    if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
    else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
    else if (s > max3) { max3 = s; ind3 = i; }
  }
  if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
  else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}

// The greedy assignment of SearchByProjection(F, MapPoints) in map-point order (src/ORBmatcher.cc:106-163) over the candidate
// lists of window_candidates: query k belongs to map point src[k] (ascending).  -> the reference's return value.
int greedy_points(const plvs_frame_view* F, const int32_t* src, size_t nq, const std::vector<int32_t>& q_at,
                  const std::vector<int32_t>& q_n, const std::vector<int32_t>& pair_t, const std::vector<int32_t>& dist, float nn_ratio,
                  const uint8_t* occupied, const uint8_t* has_obs, int32_t* assigned) {
  std::vector<uint8_t> blocked(F->n);
  for (int i = 0; i < F->n; ++i) blocked[i] = occupied ? occupied[i] : 0;
  int n = 0;
  for (size_t k = 0; k < nq; ++k) {
    if (q_n[k] == 0) continue;
    int best = 256, best2 = 256, best_level = -1, best_level2 = -1, best_idx = -1;
    for (int p = q_at[k]; p < q_at[k] + q_n[k]; ++p) {
      const int idx = pair_t[p];
      if (blocked[idx]) continue;   // F.mvpMapPoints[idx] && Observations() > 0
      const int d = dist[p];
      if (d < best) {
        best2 = best; best = d;
        best_level2 = best_level; best_level = F->octave[idx];
        best_idx = idx;
      } else if (d < best2) {
        best_level2 = F->octave[idx];
        best2 = d;
      }
    }
    if (best <= kThHigh) {
      if (best_level == best_level2 && (float)best > nn_ratio * (float)best2) continue;
      if (best_level != best_level2 || (float)best <= nn_ratio * (float)best2) {
        assigned[best_idx] = src[k];
        blocked[best_idx] = has_obs ? has_obs[src[k]] : 1;
        ++n;
      }
    }
  }
  return n;
}

// The window query of one map point in view (:82-104): RadiusByViewingCos (:246-252, a comparison in double), the th
// factor, the radius at the predicted level, GetFeaturesInArea(x, y, r, level - 1, level).  The frustum kernel of
// frame_track.hip writes the same record on the device.
__host__ __device__ inline WinQuery map_point_query(float proj_x, float proj_y, float proj_xr, float view_cos, int level, float th,
                                                    int factor, float scale_factor, int src) {
  float r = ((double)view_cos > 0.998) ? 2.5f : 4.0f;
  if (factor) r *= th;
  const float rr = r * scale_factor;
  return WinQuery{proj_x, proj_y, rr, proj_xr, level - 1, level, src, (level - 1 > 0 || level >= 0) ? 1 : 0};
}

// The window query of one last-frame point SearchByProjection(CurrentFrame, LastFrame, th, bMono) accepts (:1822-1835): the
// radius th * mvScaleFactors[octave], the predicted right coordinate u - mbf * invz, the level band of bForward / bBackward /
// neither.  The projection kernel of frame_motion.hip writes the same record on the device.
__host__ __device__ inline WinQuery last_frame_query(float u, float v, float invz, int octave, float th, float scale_factor, float mbf,
                                                     int forward, int backward, int src) {
  const float radius = th * scale_factor;   // :1826
  const int min_level = forward ? octave : (backward ? 0 : octave - 1);
  const int max_level = forward ? 2147483647 : (backward ? octave : octave + 1);
  return WinQuery{u, v, radius, u - mbf * invz, min_level, max_level, src, (min_level > 0 || max_level >= 0) ? 1 : 0};
}

// The greedy assignment of SearchByProjection(CurrentFrame, LastFrame) in last-frame order (:1842-1990) over the candidate lists
// of window_candidates — query k belongs to last-frame key point src[k] (ascending) —, with the rotation histogram and its cut.
// -> the reference's return value.
int greedy_last_frame_points(const plvs_frame_view* F, const float* cur_angle, const int32_t* src, size_t nq, const std::vector<int32_t>& q_at,
                             const std::vector<int32_t>& q_n, const std::vector<int32_t>& pair_t, const std::vector<int32_t>& dist,
                             const float* angle, const uint8_t* has_obs, int check_orientation, const uint8_t* occupied, int32_t* assigned) {
  std::vector<uint8_t> blocked(F->n);
  for (int i = 0; i < F->n; ++i) blocked[i] = occupied ? occupied[i] : 0;
  std::vector<int> hist_item, hist_bin;   // rotHist: what was pushed, in order (duplicates possible)
  const float factor = kHistoLength / 360.0f;
  int n = 0;
  for (size_t k = 0; k < nq; ++k) {
    if (q_n[k] == 0) continue;
    const int i = src[k];
    int best = 256, best_idx = -1;
    for (int p = q_at[k]; p < q_at[k] + q_n[k]; ++p) {
      const int i2 = pair_t[p];
      if (blocked[i2]) continue;   // CurrentFrame.mvpMapPoints[i2] && Observations() > 0
      if (dist[p] < best) { best = dist[p]; best_idx = i2; }
    }
    if (best <= kThHigh) {
      assigned[best_idx] = i;
      blocked[best_idx] = has_obs ? has_obs[i] : 1;
      ++n;
      if (check_orientation) {
        float rot = angle[i] - cur_angle[best_idx];
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
    for (int b : hist_bin) ++count[b];
    int ind1, ind2, ind3;
    three_maxima(count, kHistoLength, ind1, ind2, ind3);
    for (size_t k = 0; k < hist_bin.size(); ++k)
      if (hist_bin[k] != ind1 && hist_bin[k] != ind2 && hist_bin[k] != ind3) {
        assigned[hist_item[k]] = -1;
        --n;
      }
  }
  return n;
}

}  // namespace
}  // namespace orbwin
}  // namespace plvs
