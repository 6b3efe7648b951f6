// The loop-closing ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (reference
// src/ORBmatcher.cc:509-615) and its overload with vpPointsKFs / vpMatchedKF (:617-730) over resident key frames, as
// LoopClosing::DetectCommonRegionsFromBoW and FindMatchesByProjection call them (src/LoopClosing.cc:912/923, :956/965, :1237/1245):
// K (key frame, Scw) pairs x ONE list of M map points in one call — one copy in, one launch, one wait, then the greedy pass.
//
// The overloads are greedy (loop_search_pair.hpp): a member an earlier point took is left out.  The device does the order-free part.
// The front is the Sim3 Fuse sieve's (orb_fuse.hip): a workgroup takes a tile of 256 consecutive points of ONE key frame, a thread
// per pair through front() with the projection policy, the survivors listed in LDS by ballot and wave counts; then a wave per
// survivor walks its window.  The walk does not reduce to one key: every lane keeps the kListLen smallest keys
// (distance << kPosBits | enumeration position) it saw among the banded members at or below the cut, sorted, in registers; kListLen
// rounds of cross-lane minimum, each popped from the lane that owns it, give the wave's kListLen smallest in the reference's
// visiting order among equal distances (keys are distinct: positions are).  Lane 0 posts the pair's head (flags, count, the
// distances) and, if there is an entry, its indices.  After the wait the host runs greedy_keyframe per key frame.
#include <cstring>
#include <vector>

#include "common.hpp"
#include "fuse_jobs.hpp"
#include "keyframe_handle.hpp"
#include "loop_search_list.hpp"
#include "orb_fuse_tables.hpp"

namespace {

using plvs::fusepair::Front;
using plvs::fusepair::KfConst;
using plvs::orbfuse::FusePoints;
using plvs::orbfuse::KfArrays;
using plvs::orbfuse::KfRes;
using plvs::orbwin::FrameGrid;
namespace fp = plvs::fusepair;
namespace fj = plvs::fusejob;
namespace ls = plvs::loopsearch;

static_assert((int)fp::kProjectCamera == PLVS_LOOP_PROJECT_CAMERA && (int)fp::kProjectInvz == PLVS_LOOP_PROJECT_INVZ, "plvs_hip.h's codes");

// One wave, one pair past front(): the window walk in 64-member strides, the level band, the per-lane lists (loop_search_list.hpp), the rounds
__device__ __forceinline__ void walk_list(const KfConst& K, const KfArrays& A, const FusePoints& P, int i, const Front& f, float th, int cut, int lane,
                                          uint2* __restrict__ head, int4* __restrict__ entries) {
  const float radius = th * A.sf[f.level];
  fp::Cells w;
  if (A.n == 0 || !fp::window_cells(K, f.u, f.v, radius, &w)) {
    if (lane == 0) *head = ls::pack_head(fp::kEmptyWindow, f.ambiguous, 0, 0, 0, 0, 0u);
    return;
  }
  const FrameGrid::Member* members = A.members;
  const int* start = A.start;
  const uint4* desc = A.desc;
  const uint4 qa = P.desc[2 * (size_t)i], qb = P.desc[2 * (size_t)i + 1];
  ls::LaneList list;
  list.clear();
  bool any = false, banded = false;
  uint32_t pos0 = 0;   // enumeration position of the column's first member
  for (int ix = w.c0; ix <= w.c1; ++ix) {
    const int s = start[ix * fp::kGridRows + w.r0], e = start[ix * fp::kGridRows + w.r1 + 1];
    for (int j = s + lane; j < e; j += 64) {
      const FrameGrid::Member mb = members[j];
      if (!fp::in_area(mb.x, mb.y, f.u, f.v, radius)) continue;
      any = true;
      if (!fp::candidate_gate<fp::kGateSim3>(f.u, f.v, 0.0f, f.level, mb.x, mb.y, mb.octave, -1.0f, nullptr)) continue;
      banded = true;
      const uint4 ta = desc[2 * (size_t)mb.idx], tb = desc[2 * (size_t)mb.idx + 1];
      const uint32_t d = __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                         __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
      if ((int)d > cut) continue;
      list.insert((d << ls::kPosBits) | (pos0 + (uint32_t)(j - s)), mb.idx);
    }
    pos0 += (uint32_t)(e - s);
  }
  list.post(lane, fp::kEmptyWindow, f.ambiguous, any, banded, head, entries);
}

// The sieve of orb_fuse.hip's loop_fuse_sieve_kernel with the projection policy and the list walk: grid n_kfs * ceil(m / 256), a tile
// never straddles key frames, so the key frame's table entry stays in scalar registers.  A list entry in LDS: index in the tile, u, v,
// level | ambiguous << 8.
template <fp::Projection kProjection>
__global__ __launch_bounds__(256) void loop_search_sieve_kernel(const KfRes* __restrict__ kfs, FusePoints P, float th, int cut, int tiles_per_kf,
                                                                uint2* __restrict__ heads, int4* __restrict__ entries) {
  __shared__ int4 list[256];
  __shared__ int wave_count[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / (unsigned)tiles_per_kf));
  const int tile0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x - (unsigned)k * (unsigned)tiles_per_kf) * 256);
  const KfRes& D = kfs[k];
  const int i = tile0 + tid;
  bool survivor = false;
  Front f{fp::kSkipped, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f};
  if (i < P.m) {
    const int pair = k * P.m + i;
    if (!(P.skip && P.skip[pair])) f = fp::front<kProjection>(D.k, P.pos + 3 * (size_t)i, P.normal + 3 * (size_t)i, P.min_dist[i], P.max_dist[i]);
    survivor = f.reached == fp::kEmptyWindow;
    if (!survivor) heads[pair] = ls::pack_head(f.reached, 0, 0, 0, 0, 0, 0u);
  }
  const unsigned long long mask = __ballot(survivor);
  if (lane == 0) wave_count[wave] = __popcll(mask);
  __syncthreads();
  int before = 0, total = 0;
  for (int w = 0; w < 4; ++w) {
    const int c = wave_count[w];
    before += w < wave ? c : 0;
    total += c;
  }
  if (survivor) list[before + __popcll(mask & ((1ull << lane) - 1ull))] = make_int4(tid, __float_as_int(f.u), __float_as_int(f.v), f.level | (f.ambiguous << 8));
  __syncthreads();
  total = __builtin_amdgcn_readfirstlane(total);
  for (int e = wave; e < total; e += 4) {   // e < total <= 256: inside the list
    const int4 ent = list[e];
    Front g{fp::kEmptyWindow, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f};
    const int t = __builtin_amdgcn_readfirstlane(ent.x), lv = __builtin_amdgcn_readfirstlane(ent.w);
    g.u = __int_as_float(__builtin_amdgcn_readfirstlane(ent.y));
    g.v = __int_as_float(__builtin_amdgcn_readfirstlane(ent.z));
    g.level = lv & 0xff;
    g.ambiguous = lv >> 8;
    const size_t pair = (size_t)k * P.m + tile0 + t;   // t < 256 and tile0 + t < m: a survivor passed i < P.m
    walk_list(D.k, D.a, P, tile0 + t, g, th, cut, lane, heads + pair, entries + pair);
  }
}

// The call as a part of the staging block (fuse_jobs.hpp): [KfRes table | points | skip] copied in one piece, no device scratch,
// [heads | entries] posted into the pinned side.
struct LoopSearchPoints : fj::Part {
  const plvs_keyframe* const* const kfs;
  const plvs_keyframe_sim3_pose* const sim3;
  const int n_kfs;
  const plvs_fuse_points* const P;
  const uint8_t* const skip;
  const uint8_t* const* const occupied;
  const float th;
  const int cut, projection;
  ls::HeldOutputs out;
  int32_t* const stats;
  std::vector<KfConst> consts;
  std::vector<uint8_t> claimed;
  size_t o_tab = 0, o_pos = 0, o_nrm = 0, o_mind = 0, o_maxd = 0, o_pd = 0, o_skip = 0, o_entries = 0;
  int st_host = 0, st_windows = 0, st_truncated = 0;

  LoopSearchPoints(const plvs_keyframe* const* kfs_, const plvs_keyframe_sim3_pose* sim3_, int n_kfs_, const plvs_fuse_points* P_,
                   const uint8_t* skip_, const uint8_t* const* occupied_, float th_, int cut_, int projection_, const ls::HeldOutputs& out_, int32_t* stats_)
      : kfs(kfs_), sim3(sim3_), n_kfs(n_kfs_), P(P_), skip(skip_), occupied(occupied_), th(th_), cut(cut_), projection(projection_), stats(stats_) {
    out.match_idx = out_.match_idx; out.match_dist = out_.match_dist; out.reached = out_.reached; out.nmatches = out_.nmatches;
  }

  size_t n_pairs() const { return (size_t)n_kfs * P->m; }

  void prepare() override {
    const size_t m = (size_t)P->m;
    consts.resize((size_t)n_kfs);
    for (int k = 0; k < n_kfs; ++k) consts[k] = plvs::orbfuse::sim3_const(*kfs[k], sim3[k]);
    bool work = false;   // a pair that is not skipped, in a key frame that has key points
    for (int k = 0; k < n_kfs && !work; ++k) work = kfs[k]->pt.n > 0 && fj::any_unskipped(skip ? skip + k * m : nullptr, m);
    device = work && !on_host;
    if (!device) return;
    fj::Take take;
    o_tab = take(sizeof(KfRes) * (size_t)n_kfs);
    o_pos = take(sizeof(float) * 3 * m); o_nrm = take(sizeof(float) * 3 * m);
    o_mind = take(sizeof(float) * m); o_maxd = take(sizeof(float) * m); o_pd = take(m * 32);
    o_skip = take(skip ? n_pairs() : 0);
    in_bytes = take.at;
    o_entries = fj::up16(sizeof(uint2) * n_pairs());
    out_bytes = o_entries + fj::up16(sizeof(int4) * n_pairs());
  }

  void fill(char* pinned) override {
    const size_t m = (size_t)P->m;
    char* p = pinned + in_at;
    KfRes* tab = reinterpret_cast<KfRes*>(p + o_tab);
    for (int k = 0; k < n_kfs; ++k) tab[k] = KfRes{consts[k], plvs::orbfuse::arrays_at(kfs[k]->dev, kfs[k]->pt)};
    memcpy(p + o_pos, P->pos, sizeof(float) * 3 * m);
    memcpy(p + o_nrm, P->normal, sizeof(float) * 3 * m);
    memcpy(p + o_mind, P->min_dist, sizeof(float) * m);
    memcpy(p + o_maxd, P->max_dist, sizeof(float) * m);
    memcpy(p + o_pd, P->desc, m * 32);
    if (skip) memcpy(p + o_skip, skip, n_pairs());
  }

  int launch(char* dev, char* pinned, hipStream_t stream) override {
    const char* d = dev + in_at;
    const FusePoints FP{reinterpret_cast<const float*>(d + o_pos), reinterpret_cast<const float*>(d + o_nrm),
                        reinterpret_cast<const float*>(d + o_mind), reinterpret_cast<const float*>(d + o_maxd),
                        reinterpret_cast<const uint4*>(d + o_pd), skip ? reinterpret_cast<const uint8_t*>(d + o_skip) : nullptr,
                        P->m, (int)n_pairs()};
    const KfRes* tab = reinterpret_cast<const KfRes*>(d + o_tab);
    uint2* heads = reinterpret_cast<uint2*>(pinned + out_at);
    int4* entries = reinterpret_cast<int4*>(pinned + out_at + o_entries);
    const int tiles = (int)plvs::ceil_div((size_t)P->m, 256);
    const dim3 grid((unsigned)n_kfs * (unsigned)tiles);
    if (projection == PLVS_LOOP_PROJECT_INVZ)
      hipLaunchKernelGGL(loop_search_sieve_kernel<fp::kProjectInvz>, grid, dim3(256), 0, stream, tab, FP, th, cut, tiles, heads, entries);
    else
      hipLaunchKernelGGL(loop_search_sieve_kernel<fp::kProjectCamera>, grid, dim3(256), 0, stream, tab, FP, th, cut, tiles, heads, entries);
    PLVS_KERNEL_CHECK();
    ++launches;
    return PLVS_OK;
  }

  ls::PairResult host_pair(int k, int i, const uint8_t* claimed_now) const {   // on the handle's host copy
    const KfArrays a = plvs::orbfuse::arrays_at(kfs[k]->host.data(), kfs[k]->pt);
    const fp::KfGrid<FrameGrid::Member> G{a.start, a.members, a.u_right, reinterpret_cast<const uint8_t*>(a.desc), a.sf, a.sig};
    return ls::point_pair_host(consts[k], G, projection, P->pos + 3 * (size_t)i, P->normal + 3 * (size_t)i, P->min_dist[i], P->max_dist[i],
                               P->desc + 32 * (size_t)i, th, cut, claimed_now, 0);
  }

  // every key frame's greedy pass; heads / entries: the device's records, or null: every pair is the host's
  void greedy(const uint2* heads, const int4* entries) {
    const int m = P->m;
    out.reserve(n_pairs(), n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
      const size_t at = (size_t)k * m;
      claimed.assign((size_t)kfs[k]->pt.n, 0);
      if (occupied && occupied[k])
        for (size_t j = 0; j < claimed.size(); ++j) claimed[j] = occupied[k][j] != 0;
      const uint8_t* sk = skip ? skip + at : nullptr;
      const ls::GreedyCounts n = ls::greedy_keyframe(
          m, ls::point_codes(),
          [&](int i) {
            if (heads) return ls::unpack(heads[at + i], entries[at + i]);
            ls::PairList L{};
            L.reached = fp::kSkipped;
            L.host = !(sk && sk[i]);
            return L;
          },
          [&](int i, const uint8_t* c) { return host_pair(k, i, c); }, claimed.data(), out.idx.get() + at, out.dist.get() + at,
          out.code.get() + at);
      out.n[k] = n.matches;
      if (heads) st_host += n.host_pairs;
      st_truncated += n.truncated_pairs;
      st_windows += n.windows;
    }
  }

  void host_all() override { greedy(nullptr, nullptr); }
  void collect(const char* pinned) override {
    greedy(reinterpret_cast<const uint2*>(pinned + out_at), reinterpret_cast<const int4*>(pinned + out_at + o_entries));
  }
  void post() override {
    out.write();
    if (!stats) return;
    stats[0] = st_host; stats[1] = st_windows; stats[2] = launches; stats[3] = fj::copy_in_stat(*this); stats[4] = st_truncated;
  }
};

}  // namespace

int plvs::fusejob::make_loop_search_point_part(const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3, int n_kfs,
                                               const plvs_fuse_points* P, const uint8_t* skip, const uint8_t* const* occupied, float th,
                                               float ratio_hamming, int projection, int32_t* match_idx, int32_t* match_dist, uint8_t* reached,
                                               int32_t* nmatches, int32_t* stats, bool host_entry, std::unique_ptr<Part>* out) {
  out->reset();
  int rc = check_common(kfs, n_kfs, P ? P->m : -1, P && P->pos && P->normal && P->min_dist && P->max_dist && P->desc, th, match_idx, match_dist,
                        "null points / negative size", "null map point array");
  if (rc != PLVS_OK) return rc;
  int cut = 0;
  const ls::Refusal cr = ls::threshold_cut(ls::kPointThLow, ratio_hamming, &cut);
  PLVS_REQUIRE(cr != ls::kCutBadRatio, "ratio_hamming negative or NaN");
  PLVS_REQUIRE(cr == ls::kCutOk, "TH_LOW * ratio_hamming >= 256: a point without a candidate would write vpMatched[-1]");
  PLVS_REQUIRE(projection == PLVS_LOOP_PROJECT_CAMERA || projection == PLVS_LOOP_PROJECT_INVZ, "unknown projection");
  rc = check_handles(kfs, sim3, n_kfs, 1, host_entry);
  if (rc != PLVS_OK) return rc;
  ls::HeldOutputs held;
  held.match_idx = match_idx; held.match_dist = match_dist; held.reached = reached; held.nmatches = nmatches;
  if (n_kfs > 0 && P->m > 0)
    out->reset(new LoopSearchPoints(kfs, sim3, n_kfs, P, skip, occupied, th, cut, projection, held, stats));
  return PLVS_OK;
}
