// The loop-closing LineMatcher::SearchByProjection(pKF, Scw, vpLines, vpMatched, th, ratioHamming) (reference
// src/LineMatcher.cc:1767-1909) and its overload with vpLinesKFs / vpMatchedKF (:1913-2037) over resident key frames, as
// LoopClosing::DetectCommonRegionsFromBoW and FindMatchesByProjection call them (src/LoopClosing.cc:923, :965, :1245): K (key frame,
// Scw) pairs x ONE list of M map lines in one call — one copy in, one launch, one wait, then the greedy pass.
//
// The front and the window are the Sim3 Fuse's (line_fuse.hip: a wave per pair — there are few lines and the front is the larger
// part of the work; theta's plan and its ambiguity as there); the candidate gate is the level band alone (kGateBand), and the walk
// keeps lists instead of one key (loop_search_list.hpp), as orb_loop_search.hip does for points.  A pair whose level or theta the
// host must decide is posted as such and evaluated by the host at its turn in the greedy pass; a pair that asks for the full theta
// interval refuses the call before any output is written.
#include <cstring>
#include <vector>

#include "common.hpp"
#include "fuse_jobs.hpp"
#include "keyframe_handle.hpp"
#include "line_fuse_tables.hpp"
#include "loop_search_list.hpp"

namespace {

namespace lf = plvs::linefuse;
namespace fj = plvs::fusejob;
namespace ls = plvs::loopsearch;
using lf::Front;
using lf::KfConst;
using lf::Member;
using plvs::linefusetab::FuseLines;
using plvs::linefusetab::KfArrays;
using plvs::linefusetab::KfRes;

// One wave, one pair past front(): line_fuse.hip's walk_pair with the band gate, the cut and the lists
__device__ __forceinline__ void walk_list(const KfConst& K, const KfArrays& A, const FuseLines& L, int i, const Front& f, float th, int cut, int lane,
                                          uint2* __restrict__ head, int4* __restrict__ entries) {
  if (f.reached != lf::kEmptyWindow) {
    if (lane == 0) *head = ls::pack_head(f.reached, 0, 0, 0, 0, 0, 0u);
    return;
  }
  // :1841-1844 and the head of GetLineFeaturesInArea, uniform across the wave
  const float scale = A.sf[f.level];
  const float dtheta = (float)(10 * lf::kPi / 180.f) * scale;
  const float dd = th * 100.0f * scale;
  const float theta = lf::theta_device(f.rep);
  const lf::ThetaPlan plan = lf::theta_plan(K, theta, dtheta);
  const int ambiguous = (f.ambiguous || plan.nested || lf::theta_ambiguous(K, theta, dtheta, plan)) ? 1 : 0;
  if (ambiguous || plan.full || A.n_members == 0) {   // (the host decides; the refusal; nothing to walk)
    if (lane == 0) *head = ls::pack_head(plan.full && !ambiguous ? lf::kFullTheta : lf::kEmptyWindow, ambiguous, 0, 0, 0, 0, 0u);
    return;
  }
  const Member* members = A.members;
  const int* start = A.start;
  const uint4* desc = A.desc;
  const uint4 qa = L.desc[2 * (size_t)i], qb = L.desc[2 * (size_t)i + 1];
  const lf::Rep none{0.0f, 0.0f, 0.0f};
  const float dmin = f.rep.d - dd, dmax = f.rep.d + dd;
  ls::LaneList list;
  list.clear();
  bool banded = false;
  uint32_t pos0 = 0;   // enumeration position of the range's first member; it runs on across the sub-windows
  for (int s = 0; s < plan.n; ++s) {
    const lf::Cells c = lf::leaf_cells(K, lf::plan_leaf(plan, s, dmin, dmax));
    if (!c.ok) continue;
    for (int ix = c.c0; ix <= c.c1; ++ix) {   // c0 >= 0, c1 <= kCols - 1, 0 <= r0, r1 <= kRows - 1: inside the kCols * kRows + 1 starts
      const int a = start[ix * lf::kRows + c.r0], e = start[ix * lf::kRows + c.r1 + 1];
      for (int j = a + lane; j < e; j += 64) {
        const Member mb = members[j];
        if (!lf::candidate_gate<lf::kGateBand>(f.rep, none, f.level, mb, nullptr)) continue;
        banded = true;
        const uint4 ta = desc[2 * (size_t)mb.idx], tb = desc[2 * (size_t)mb.idx + 1];
        const uint32_t d = __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                           __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
        if ((int)d > cut) continue;
        list.insert((d << ls::kPosBits) | (pos0 + (uint32_t)(j - a)), mb.idx);
      }
      if (e > a) pos0 += (uint32_t)(e - a);
    }
  }
  list.post(lane, lf::kEmptyWindow, 0, pos0 > 0, banded, head, entries);   // pos0 > 0: vIndices is not empty
}

// The resident layout of line_fuse.hip: the pair index is the wave's, taken through readfirstlane, so the pair's table entry is read
// by scalar loads.
__global__ __launch_bounds__(256) void line_loop_search_kernel(const KfRes* __restrict__ kfs, FuseLines L, float th, int cut, uint2* __restrict__ heads,
                                                               int4* __restrict__ entries) {
  const int lane = threadIdx.x & 63;
  const int pair = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (pair >= L.n_pairs) return;
  const int k = pair / L.m, i = pair - k * L.m;
  if (L.skip && L.skip[pair]) {
    if (lane == 0) heads[pair] = ls::pack_head(lf::kSkipped, 0, 0, 0, 0, 0, 0u);
    return;
  }
  const KfRes& D = kfs[k];
  const Front f = lf::front(D.k, L.start + 3 * (size_t)i, L.end + 3 * (size_t)i, L.normal + 3 * (size_t)i, L.max_dist[i]);
  walk_list(D.k, D.a, L, i, f, th, cut, lane, heads + pair, entries + pair);
}

const char* const kFullThetaMessage =
    "GetLineFeaturesInArea: search over the full theta interval (deltaTheta above pi / 2: the reference terminates here)";

// The call as a part of the staging block (fuse_jobs.hpp): [KfRes table | lines | skip] copied in one piece, no device scratch,
// [heads | entries] posted into the pinned side.
struct LoopSearchLines : fj::Part {
  const plvs_keyframe* const* const kfs;
  const plvs_keyframe_sim3_pose* const sim3;
  const int n_kfs;
  const plvs_fuse_lines* const L;
  const uint8_t* const skip;
  const uint8_t* const* const occupied;
  const float th;
  const int cut;
  ls::HeldOutputs out;
  int32_t* const stats;
  std::vector<KfConst> consts;
  std::vector<uint8_t> claimed;
  size_t o_tab = 0, o_start = 0, o_end = 0, o_nrm = 0, o_maxd = 0, o_desc = 0, o_skip = 0, o_entries = 0;
  int st_host = 0, st_windows = 0, st_truncated = 0;

  LoopSearchLines(const plvs_keyframe* const* kfs_, const plvs_keyframe_sim3_pose* sim3_, int n_kfs_, const plvs_fuse_lines* L_, const uint8_t* skip_,
                  const uint8_t* const* occupied_, float th_, int cut_, const ls::HeldOutputs& out_, int32_t* stats_)
      : kfs(kfs_), sim3(sim3_), n_kfs(n_kfs_), L(L_), skip(skip_), occupied(occupied_), th(th_), cut(cut_), stats(stats_) {
    out.match_idx = out_.match_idx; out.match_dist = out_.match_dist; out.reached = out_.reached; out.nmatches = out_.nmatches;
  }

  size_t n_pairs() const { return (size_t)n_kfs * L->m; }

  void prepare() override {
    const size_t m = (size_t)L->m;
    consts.resize((size_t)n_kfs);
    for (int k = 0; k < n_kfs; ++k) consts[k] = plvs::linefusetab::sim3_const(*kfs[k], sim3[k]);
    bool any_lines = false;   // a pair that is not skipped, and a key frame that has key lines
    for (int k = 0; k < n_kfs && !any_lines; ++k) any_lines = kfs[k]->ln.n > 0;
    device = any_lines && fj::any_unskipped(skip, n_pairs()) && !on_host;
    if (!device) return;
    fj::Take take;
    o_tab = take(sizeof(KfRes) * (size_t)n_kfs);
    o_start = take(sizeof(float) * 3 * m); o_end = take(sizeof(float) * 3 * m); o_nrm = take(sizeof(float) * 3 * m);
    o_maxd = take(sizeof(float) * m); o_desc = take(m * 32);
    o_skip = take(skip ? n_pairs() : 0);
    in_bytes = take.at;
    o_entries = fj::up16(sizeof(uint2) * n_pairs());
    out_bytes = o_entries + fj::up16(sizeof(int4) * n_pairs());
  }

  void fill(char* pinned) override {
    const size_t m = (size_t)L->m;
    char* p = pinned + in_at;
    KfRes* tab = reinterpret_cast<KfRes*>(p + o_tab);
    for (int k = 0; k < n_kfs; ++k) tab[k] = KfRes{consts[k], plvs::linefusetab::arrays_at(kfs[k]->dev, kfs[k]->ln)};
    memcpy(p + o_start, L->start, sizeof(float) * 3 * m);
    memcpy(p + o_end, L->end, sizeof(float) * 3 * m);
    memcpy(p + o_nrm, L->normal, sizeof(float) * 3 * m);
    memcpy(p + o_maxd, L->max_dist, sizeof(float) * m);
    memcpy(p + o_desc, L->desc, m * 32);
    if (skip) memcpy(p + o_skip, skip, n_pairs());
  }

  int launch(char* dev, char* pinned, hipStream_t stream) override {
    const char* d = dev + in_at;
    const FuseLines FL{reinterpret_cast<const float*>(d + o_start), reinterpret_cast<const float*>(d + o_end),
                       reinterpret_cast<const float*>(d + o_nrm), reinterpret_cast<const float*>(d + o_maxd),
                       reinterpret_cast<const uint4*>(d + o_desc), skip ? reinterpret_cast<const uint8_t*>(d + o_skip) : nullptr,
                       L->m, (int)n_pairs()};
    hipLaunchKernelGGL(line_loop_search_kernel, dim3(plvs::ceil_div(n_pairs(), 4)), dim3(256), 0, stream,
                       reinterpret_cast<const KfRes*>(d + o_tab), FL, th, cut, reinterpret_cast<uint2*>(pinned + out_at),
                       reinterpret_cast<int4*>(pinned + out_at + o_entries));
    PLVS_KERNEL_CHECK();
    ++launches;
    return PLVS_OK;
  }

  ls::PairResult host_pair(int k, int i, const uint8_t* claimed_now) const {   // on the handle's host copy
    const KfArrays a = plvs::linefusetab::arrays_at(kfs[k]->host.data(), kfs[k]->ln);
    const lf::KfGrid G{a.start, a.members, reinterpret_cast<const uint8_t*>(a.desc), a.sf, a.sig};
    return ls::line_pair_host(consts[k], G, L->start + 3 * (size_t)i, L->end + 3 * (size_t)i, L->normal + 3 * (size_t)i, L->max_dist[i],
                              L->desc + 32 * (size_t)i, th, cut, claimed_now, 0, 0);
  }

  // every key frame's greedy pass; heads / entries: the device's records, or null: every pair is the host's
  void greedy(const uint2* heads, const int4* entries) {
    const int m = L->m;
    out.reserve(n_pairs(), n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
      const size_t at = (size_t)k * m;
      claimed.assign((size_t)kfs[k]->ln.n, 0);
      if (occupied && occupied[k])
        for (size_t j = 0; j < claimed.size(); ++j) claimed[j] = occupied[k][j] != 0;
      const uint8_t* sk = skip ? skip + at : nullptr;
      const ls::GreedyCounts n = ls::greedy_keyframe(
          m, ls::line_codes(),
          [&](int i) {
            if (heads) return ls::unpack(heads[at + i], entries[at + i]);
            ls::PairList P{};
            P.reached = lf::kSkipped;
            P.host = !(sk && sk[i]);
            return P;
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
  int refused() override {   // nothing is written when a pair asks for the full theta interval
    for (size_t p = 0; p < out.pairs; ++p)
      if (out.code[p] == lf::kFullTheta) {
        plvs::set_error("invalid argument: %s", kFullThetaMessage);
        return PLVS_ERR_INVALID_ARG;
      }
    return PLVS_OK;
  }
  void post() override {
    out.write();
    if (!stats) return;
    stats[0] = st_host; stats[1] = st_windows; stats[2] = launches; stats[3] = fj::copy_in_stat(*this); stats[4] = st_truncated;
  }
};

}  // namespace

int plvs::fusejob::make_loop_search_line_part(const plvs_keyframe* const* kfs, const plvs_keyframe_sim3_pose* sim3, int n_kfs, const plvs_fuse_lines* L,
                                              const uint8_t* skip, const uint8_t* const* occupied, float th, float ratio_hamming, int32_t* match_idx,
                                              int32_t* match_dist, uint8_t* reached, int32_t* nmatches, int32_t* stats, bool host_entry,
                                              std::unique_ptr<Part>* out) {
  out->reset();
  int rc = check_common(kfs, n_kfs, L ? L->m : -1, L && L->start && L->end && L->normal && L->max_dist && L->desc, th, match_idx, match_dist,
                        "null lines / negative size", "null map line array");
  if (rc != PLVS_OK) return rc;
  int cut = 0;
  const ls::Refusal cr = ls::threshold_cut(ls::kLineThLow, ratio_hamming, &cut);
  PLVS_REQUIRE(cr != ls::kCutBadRatio, "ratio_hamming negative or NaN");
  PLVS_REQUIRE(cr == ls::kCutOk, "TH_LOW * ratio_hamming >= 256: no descriptor distance lies above the threshold");
  rc = check_handles(kfs, sim3, n_kfs, 2, host_entry);
  if (rc != PLVS_OK) return rc;
  ls::HeldOutputs held;
  held.match_idx = match_idx; held.match_dist = match_dist; held.reached = reached; held.nmatches = nmatches;
  if (n_kfs > 0 && L->m > 0) out->reset(new LoopSearchLines(kfs, sim3, n_kfs, L, skip, occupied, th, cut, held, stats));
  return PLVS_OK;
}
