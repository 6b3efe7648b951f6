// The search stage of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight = false) (reference src/ORBmatcher.cc:1244-1434) as
// LocalMapping::SearchInNeighbors calls it (src/LocalMapping.cc:1372-1410): K key frames x M map points in ONE call — one copy in,
// one launch (two in the chained layout), one wait.  Single-camera pinhole key frames only (NLeft == -1).
//
// Fuse has no greedy pass: a pair's result depends on nobody else's.  A wave takes one (key frame, point) pair; the projection and
// the tests of fuse_pair.hpp are uniform across it and a rejected pair leaves at once; an accepted pair walks its window columns in
// 64-member strides (the CSR grid of orb_window.hpp), every lane keeping the smallest (distance, enumeration position) it has
// seen; one cross-lane minimum, and lane 0 posts the pair's record straight into the pinned block.  No candidate list, no spill.
//
// The level needs the host's logarithm (track_level.hpp): the pairs predict_level marks ambiguous are evaluated once more by the
// host entry's code after the wait, and their result is simply the host's.
//
// Map mutation (AddObservation, AddMapPoint, Replace) stays the caller's: INTEGRATION.md has the replay.
//
// The Sim3 overload of LoopClosing::SearchAndFuse (src/ORBmatcher.cc:1437-1553, fuse_pair.hpp's kGateSim3) runs over resident key
// frames only, in one of two layouts: the wave-per-pair kernel above with the other gate, or the sieve (loop_fuse_sieve_kernel) —
// a loop's points are spread over many key frames' views, most pairs die in front(), and a wave per pair spends 64 lanes on each
// such rejection.  The sieve gives a THREAD to every pair first and a wave only to the survivors.
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "fuse_jobs.hpp"
#include "fuse_pair.hpp"
#include "keyframe_handle.hpp"
#include "orb_fuse_tables.hpp"
#include "orb_window.hpp"

namespace {

using plvs::fusepair::Front;
using plvs::fusepair::KfConst;
using plvs::orbfuse::arrays_at;
using plvs::orbfuse::FusePoints;
using plvs::orbfuse::KfArrays;
using plvs::orbfuse::KfRes;
using plvs::orbfuse::kPosBits;
using plvs::orbwin::FrameGrid;
namespace fp = plvs::fusepair;
namespace fj = plvs::fusejob;

constexpr int kMaxLevels = 64;

// one key frame in the staged block: the constants and where its arrays start (bytes from the block's start)
struct KfDev {
  KfConst k;
  int n, pad;
  unsigned long long o_mem, o_start, o_ur, o_desc, o_sf, o_sig;
};

// the record a pair posts: best_idx, and best_dist (16 bits, 0xffff = -1) | reached << 16 | ambiguous << 24
__host__ __device__ inline int2 pack(int best_idx, int best_dist, int reached, int ambiguous) {
  return make_int2(best_idx, (best_dist & 0xffff) | (reached << 16) | (ambiguous << 24));
}

// the chained layout's front kernel: a thread per pair, :1294-1337
__global__ __launch_bounds__(256) void fuse_front_kernel(const KfDev* __restrict__ kfs, FusePoints P, Front* __restrict__ fronts) {
  const int pair = blockIdx.x * 256 + threadIdx.x;
  if (pair >= P.n_pairs) return;
  const int k = pair / P.m, i = pair - k * P.m;
  Front f{fp::kSkipped, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f};
  if (!(P.skip && P.skip[pair])) f = fp::front(kfs[k].k, P.pos + 3 * (size_t)i, P.normal + 3 * (size_t)i, P.min_dist[i], P.max_dist[i]);
  fronts[pair] = f;
}

// One wave, one pair past the tests of front(): the window walk in 64-member strides, the gates, the (distance, enumeration position)
// key, the cross-lane minimum and the posted record.  ONE text: the staged kernel and the resident kernel both call it.
template <fp::Gate kGate>
__device__ __forceinline__ void walk_pair(const KfConst& K, const KfArrays& A, const FusePoints& P, int i, const Front& f, float th, int lane,
                                          int2* __restrict__ rec) {
  if (f.reached != fp::kEmptyWindow) {
    if (lane == 0) *rec = pack(-1, -1, f.reached, 0);
    return;
  }
  const float radius = th * A.sf[f.level];
  fp::Cells w;
  if (A.n == 0 || !fp::window_cells(K, f.u, f.v, radius, &w)) {
    if (lane == 0) *rec = pack(-1, -1, fp::kEmptyWindow, f.ambiguous);
    return;
  }
  const FrameGrid::Member* members = A.members;
  const int* start = A.start;
  const float* u_right = A.u_right;
  const uint4* desc = A.desc;
  const float* sig = A.sig;
  const uint4 qa = P.desc[2 * (size_t)i], qb = P.desc[2 * (size_t)i + 1];
  uint32_t best = 0xffffffffu;
  int best_idx = -1;
  bool any = false, gated = false;
  uint32_t pos0 = 0;   // enumeration position of the column's first member
  for (int ix = w.c0; ix <= w.c1; ++ix) {
    const int s = start[ix * fp::kGridRows + w.r0], e = start[ix * fp::kGridRows + w.r1 + 1];
    for (int j = s + lane; j < e; j += 64) {
      const FrameGrid::Member mb = members[j];
      if (!fp::in_area(mb.x, mb.y, f.u, f.v, radius)) continue;
      any = true;
      if (!fp::candidate_gate<kGate>(f.u, f.v, f.ur, f.level, mb.x, mb.y, mb.octave, kGate == fp::kGateSE3 ? u_right[mb.idx] : -1.0f, sig)) continue;
      gated = true;
      const uint4 ta = desc[2 * (size_t)mb.idx], tb = desc[2 * (size_t)mb.idx + 1];
      const uint32_t d = __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                         __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
      const uint32_t key = (d << kPosBits) | (pos0 + (uint32_t)(j - s));
      if (key < best) { best = key; best_idx = mb.idx; }
    }
    pos0 += (uint32_t)(e - s);
  }
  // one reduction: the smallest key is the first minimum in enumeration order; keys are distinct
  uint32_t lowest = best;
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)lowest, off);
    lowest = o < lowest ? o : lowest;
  }
  const unsigned long long has_any = __ballot(any), has_gated = __ballot(gated);
  const unsigned long long owner = __ballot(gated && best == lowest);
  int win_idx = -1;
  if (owner) win_idx = __shfl(best_idx, __ffsll((long long)owner) - 1);
  if (lane == 0) {
    int reached = fp::kEmptyWindow, idx = -1, dist = -1;
    if (has_any) {
      const int d = (int)(lowest >> kPosBits);
      reached = !has_gated ? fp::kNoCandidate : (d <= fp::kThLow ? fp::kCandidate : fp::kAboveThLow);
      if (reached == fp::kCandidate) { idx = win_idx; dist = d; }
    }
    *rec = pack(idx, dist, reached, f.ambiguous);
  }
}

template <bool kChained>
__global__ __launch_bounds__(256) void fuse_window_kernel(const char* __restrict__ base, const KfDev* __restrict__ kfs, FusePoints P, float th,
                                                          const Front* __restrict__ fronts, int2* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= P.n_pairs) return;
  const int k = pair / P.m, i = pair - k * P.m;
  Front f;
  if (kChained) {
    f = fronts[pair];
  } else {
    if (P.skip && P.skip[pair]) {
      if (lane == 0) out[pair] = pack(-1, -1, fp::kSkipped, 0);
      return;
    }
    f = fp::front(kfs[k].k, P.pos + 3 * (size_t)i, P.normal + 3 * (size_t)i, P.min_dist[i], P.max_dist[i]);
  }
  const KfDev& D = kfs[k];
  const KfArrays A{reinterpret_cast<const FrameGrid::Member*>(base + D.o_mem), reinterpret_cast<const int*>(base + D.o_start),
                   reinterpret_cast<const float*>(base + D.o_ur), reinterpret_cast<const uint4*>(base + D.o_desc),
                   reinterpret_cast<const float*>(base + D.o_sf), reinterpret_cast<const float*>(base + D.o_sig), D.n};
  walk_pair<fp::kGateSE3>(D.k, A, P, i, f, th, lane, out + pair);
}

// The resident layout: the table holds pointers into the handles' own allocations (keyframe_handle.hpp), nothing of a key frame is in
// the call's block.  The pair index is the wave's: taken through readfirstlane, so the compiler knows it uniform and the pair's table
// entry — pose, constants, pointers — is read by scalar loads and stays in scalar registers.
template <fp::Gate kGate>
__global__ __launch_bounds__(256) void fuse_window_resident_kernel(const KfRes* __restrict__ kfs, FusePoints P, float th, int2* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int pair = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (pair >= P.n_pairs) return;
  const int k = pair / P.m, i = pair - k * P.m;
  if (P.skip && P.skip[pair]) {
    if (lane == 0) out[pair] = pack(-1, -1, fp::kSkipped, 0);
    return;
  }
  const KfRes& D = kfs[k];
  const Front f = fp::front(D.k, P.pos + 3 * (size_t)i, P.normal + 3 * (size_t)i, P.min_dist[i], P.max_dist[i]);
  walk_pair<kGate>(D.k, D.a, P, i, f, th, lane, out + pair);
}

// The sieve layout of the Sim3 search.  A workgroup takes a tile of 256 consecutive points of ONE key frame (grid: n_kfs *
// ceil(m / 256), a tile never straddles key frames), so the key frame is the workgroup's: its table entry stays in scalar registers.
//   phase 1, a thread per pair: skip and front(); a rejected pair posts its record at once (consecutive threads, consecutive
//     records); a survivor goes to a list in LDS — its place from the wave's ballot and the four waves' counts, no atomics, so the
//     list is in tile order whatever the scheduling;
//   phase 2, a wave per survivor: wave w takes entries w, w + 4, ... through walk_pair, the text of the other layout.
// A list entry: index in the tile, u, v, level | ambiguous << 8 (16 B x 256 = 4 KiB).  ur is not kept: the Sim3 gate does not read it.
__global__ __launch_bounds__(256) void loop_fuse_sieve_kernel(const KfRes* __restrict__ kfs, FusePoints P, float th, int tiles_per_kf,
                                                              int2* __restrict__ out) {
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
    if (!(P.skip && P.skip[pair])) f = fp::front(D.k, P.pos + 3 * (size_t)i, P.normal + 3 * (size_t)i, P.min_dist[i], P.max_dist[i]);
    survivor = f.reached == fp::kEmptyWindow;
    if (!survivor) out[pair] = pack(-1, -1, f.reached, 0);
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
    walk_pair<fp::kGateSim3>(D.k, D.a, P, tile0 + t, g, th, lane, out + (k * P.m + tile0 + t));
  }
}

// pose = false: a handle's constants, the pose left at 0 (a resident call puts its own there)
KfConst kf_const(const plvs_fuse_keyframe& kf, bool pose = true) {
  KfConst c;
  for (int i = 0; i < 4; ++i) c.q[i] = pose ? kf.q_cw[i] : 0.0f;
  for (int i = 0; i < 3; ++i) { c.t[i] = pose ? kf.tcw[i] : 0.0f; c.Ow[i] = pose ? kf.Ow[i] : 0.0f; }
  c.fx = kf.K4[0]; c.fy = kf.K4[1]; c.cx = kf.K4[2]; c.cy = kf.K4[3];
  c.mbf = kf.mbf;
  c.min_x = kf.bounds4[0]; c.max_x = kf.bounds4[1]; c.min_y = kf.bounds4[2]; c.max_y = kf.bounds4[3];
  c.grid_min_x = kf.view.min_x; c.grid_min_y = kf.view.min_y;
  c.grid_w_inv = kf.view.grid_w_inv; c.grid_h_inv = kf.view.grid_h_inv;
  c.log_scale_factor = kf.log_scale_factor;
  c.n_levels = kf.n_levels;
  return c;
}

// the refusals of every entry that are not a key frame's: before anything is launched or written
int check_call(const void* kfs, int n_kfs, const plvs_fuse_points* P, float th, const int32_t* best_idx, const int32_t* best_dist) {
  return fj::check_common(kfs, n_kfs, P ? P->m : -1, P && P->pos && P->normal && P->min_dist && P->max_dist && P->desc, th, best_idx, best_dist,
                          "null points / negative size", "null map point array");
}

struct Outputs {
  int32_t *best_idx, *best_dist;
  uint8_t* reached;
  void put(size_t pair, const fp::Result& r) const {
    best_idx[pair] = r.best_idx;
    best_dist[pair] = r.best_dist;
    if (reached) reached[pair] = (uint8_t)r.reached;
  }
};

// One call's point search as a part of the staging block (fuse_jobs.hpp): everything that depends on the query and the outputs
// alone.  Where a key frame comes from is its source's, one of the two subclasses below:
// [the source's key-frame table | points | skip | what else the source stages] copied in one piece,
// [the source's scratch, HBM only], [records, posted into the pinned side]
struct PointPart : fj::Part {
  const int n_kfs;
  const plvs_fuse_points* const P;
  const uint8_t* const skip;
  const float th;
  const Outputs out;
  int32_t* const stats;
  const int n_stats;   // 4: the source writes stats[3], the bytes it put into the call's copy in
  fp::Gate gate = fp::kGateSE3;   // kGateSim3: the loop-closing overload (a resident source's)

  size_t o_tab = 0, o_pos = 0, o_nrm = 0, o_mind = 0, o_maxd = 0, o_pd = 0, o_skip = 0;   // from the part's inputs
  int st_host = 0, st_windows = 0;

  PointPart(int n_kfs_, const plvs_fuse_points* P_, const uint8_t* skip_, float th_, const Outputs& out_, int32_t* stats_, int n_stats_)
      : n_kfs(n_kfs_), P(P_), skip(skip_), th(th_), out(out_), stats(stats_), n_stats(n_stats_) {}

  // ---- the key-frame source
  virtual bool has_points(int k) const = 0;
  virtual void prepare_host() {}                  // what host_pair needs whether or not anything is launched
  virtual size_t table_entry() const = 0;         // bytes of one key frame in the table at o_tab
  virtual void size_kfs(fj::Take&) {}             // only when something is launched: what the source stages behind the query, its scratch
  virtual void fill_kfs(char* p) = 0;             // the table and what size_kfs took; p: the part's inputs in the pinned block
  virtual int launch_kfs(char* dev, const char* table, const FusePoints& FP, int2* rec, hipStream_t stream) = 0;   // launch() checks and counts its last
  virtual void host_at(int) {}                    // host_all arrives at key frame k
  virtual fp::Result host_pair(int k, int i) = 0;   // one pair on the host: pair_host() over the source's grid and constants

  fp::Result pair_host(const fp::KfGrid<FrameGrid::Member>& G, const KfConst& c, int i) const {
    const float *pos = P->pos + 3 * (size_t)i, *nrm = P->normal + 3 * (size_t)i;
    const uint8_t* d = P->desc + 32 * (size_t)i;
    return gate == fp::kGateSim3 ? fp::pair_host<fp::kGateSim3>(c, G, pos, nrm, P->min_dist[i], P->max_dist[i], d, th, 0)
                                 : fp::pair_host<fp::kGateSE3>(c, G, pos, nrm, P->min_dist[i], P->max_dist[i], d, th, 0);
  }

  size_t n_pairs() const { return (size_t)n_kfs * P->m; }

  void prepare() override {
    const size_t m = (size_t)P->m;
    prepare_host();
    // anything for the device?  a pair that is not skipped, in a key frame that has key points
    bool work = false;
    for (int k = 0; k < n_kfs && !work; ++k) work = has_points(k) && fj::any_unskipped(skip ? skip + k * m : nullptr, m);
    device = work && !on_host;
    if (!device) return;
    fj::Take take;
    o_tab = take(table_entry() * (size_t)n_kfs);
    o_pos = take(sizeof(float) * 3 * m); o_nrm = take(sizeof(float) * 3 * m);
    o_mind = take(sizeof(float) * m); o_maxd = take(sizeof(float) * m); o_pd = take(m * 32);
    o_skip = take(skip ? n_pairs() : 0);
    size_kfs(take);
    in_bytes = take.at;
    out_bytes = fj::up16(sizeof(int2) * n_pairs());
  }

  void fill(char* pinned) override {
    const size_t m = (size_t)P->m;
    char* p = pinned + in_at;
    memcpy(p + o_pos, P->pos, sizeof(float) * 3 * m);
    memcpy(p + o_nrm, P->normal, sizeof(float) * 3 * m);
    memcpy(p + o_mind, P->min_dist, sizeof(float) * m);
    memcpy(p + o_maxd, P->max_dist, sizeof(float) * m);
    memcpy(p + o_pd, P->desc, m * 32);
    if (skip) memcpy(p + o_skip, skip, n_pairs());
    fill_kfs(p);
  }

  int launch(char* dev, char* pinned, hipStream_t stream) override {
    const char* d = dev + in_at;
    const FusePoints FP{reinterpret_cast<const float*>(d + o_pos), reinterpret_cast<const float*>(d + o_nrm),
                        reinterpret_cast<const float*>(d + o_mind), reinterpret_cast<const float*>(d + o_maxd),
                        reinterpret_cast<const uint4*>(d + o_pd), skip ? reinterpret_cast<const uint8_t*>(d + o_skip) : nullptr,
                        P->m, (int)n_pairs()};
    const int rc = launch_kfs(dev, d + o_tab, FP, reinterpret_cast<int2*>(pinned + out_at), stream);
    if (rc != PLVS_OK) return rc;
    PLVS_KERNEL_CHECK();
    ++launches;
    return PLVS_OK;
  }

  // nothing launched: every pair is still reported (a key frame without key points: the tests, then an empty window)
  void host_all() override {
    const int m = P->m;
    for (int k = 0; k < n_kfs; ++k) {
      host_at(k);
      for (int i = 0; i < m; ++i) {
        const size_t pair = (size_t)k * m + i;
        const fp::Result r = (skip && skip[pair]) ? fp::Result{-1, -1, fp::kSkipped} : host_pair(k, i);
        out.put(pair, r);
        if (r.reached >= fp::kEmptyWindow) ++st_windows;
      }
    }
  }

  void collect(const char* pinned) override {
    const int m = P->m, K = n_kfs;
    const int2* rec = reinterpret_cast<const int2*>(pinned + out_at);
    const Outputs o = out;            // (locals: the stores through the output pointers may alias this object's members)
    int host = 0, windows = 0;
    for (int k = 0; k < K; ++k)
      for (int i = 0; i < m; ++i) {
        const size_t pair = (size_t)k * m + i;
        const fj::Record r = fj::unpack(rec[pair]);
        fp::Result res{r.idx, r.dist, r.reached};
        if (r.ambiguous) {   // the level is the host's to decide: the pair once more, by the host entry's code
          res = host_pair(k, i);
          ++host;
        }
        o.put(pair, res);
        if (res.reached >= fp::kEmptyWindow) ++windows;
      }
    st_host += host;
    st_windows += windows;
  }

  void post() override {
    if (!stats) return;
    stats[0] = st_host; stats[1] = st_windows; stats[2] = launches;
    if (n_stats == 4) stats[3] = fj::copy_in_stat(*this);
  }
};

// test / measurement hook.  1: the projection in a launch of its own in front of the windows; 2: the copy in alone
thread_local int g_chained = 0;
// test / measurement hook of the Sim3 search.  0: the sieve, 1: a wave per pair
thread_local int g_loop_layout = 0;

// Key frames staged per call: a KfDev table, and behind the query every key frame's members, cell starts, u_right, descriptors and
// levels; the fronts of the chained layout are its scratch
struct StagedPoints : PointPart {
  const plvs_fuse_keyframe* const kfs;
  const int chained;
  std::vector<FrameGrid> grids;   // launched: every key frame's, built only then.  host_all: the one of the key frame it is at
  std::vector<KfDev> tab;         // the same, for the constants

  StagedPoints(const plvs_fuse_keyframe* kfs_, int n_kfs_, const plvs_fuse_points* P_, const uint8_t* skip_, float th_, const Outputs& out_,
               int32_t* stats_)
      : PointPart(n_kfs_, P_, skip_, th_, out_, stats_, 3), kfs(kfs_), chained(g_chained) {}

  bool has_points(int k) const override { return kfs[k].view.n > 0; }
  size_t table_entry() const override { return sizeof(KfDev); }

  void size_kfs(fj::Take& take) override {
    grids.reserve((size_t)n_kfs);
    for (int k = 0; k < n_kfs; ++k) grids.emplace_back(&kfs[k].view);
    tab.resize((size_t)n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
      KfDev& D = tab[k];
      D.k = kf_const(kfs[k]);
      D.n = kfs[k].view.n;
      D.pad = 0;
      D.o_mem = take(sizeof(FrameGrid::Member) * (size_t)D.n);
      D.o_start = take(D.n ? sizeof(int) * grids[k].start.size() : 0);
      D.o_ur = take(sizeof(float) * (size_t)D.n);
      D.o_desc = take((size_t)D.n * 32);
      D.o_sf = take(sizeof(float) * (size_t)kfs[k].n_levels);
      D.o_sig = take(sizeof(float) * (size_t)kfs[k].n_levels);
    }
    scratch_bytes = chained == 1 ? fj::up16(sizeof(Front) * n_pairs()) : 0;
  }

  void fill_kfs(char* p) override {
    std::vector<KfDev> abs_tab = tab;   // the kernel reads a key frame's arrays at offsets from the BLOCK's start
    for (KfDev& D : abs_tab) { D.o_mem += in_at; D.o_start += in_at; D.o_ur += in_at; D.o_desc += in_at; D.o_sf += in_at; D.o_sig += in_at; }
    memcpy(p + o_tab, abs_tab.data(), sizeof(KfDev) * (size_t)n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
      const KfDev& D = tab[k];
      const plvs_fuse_keyframe& kf = kfs[k];
      if (D.n) {
        memcpy(p + D.o_mem, grids[k].members.data(), sizeof(FrameGrid::Member) * (size_t)D.n);
        memcpy(p + D.o_start, grids[k].start.data(), sizeof(int) * grids[k].start.size());
        memcpy(p + D.o_ur, kf.view.u_right, sizeof(float) * (size_t)D.n);
        memcpy(p + D.o_desc, kf.view.desc, (size_t)D.n * 32);
      }
      memcpy(p + D.o_sf, kf.view.scale_factors, sizeof(float) * (size_t)kf.n_levels);
      memcpy(p + D.o_sig, kf.inv_level_sigma2, sizeof(float) * (size_t)kf.n_levels);
    }
  }

  int launch_kfs(char* dev, const char* table, const FusePoints& FP, int2* rec, hipStream_t stream) override {
    const KfDev* dtab = reinterpret_cast<const KfDev*>(table);
    if (chained == 1) {
      Front* fronts = reinterpret_cast<Front*>(dev + scratch_at);
      hipLaunchKernelGGL(fuse_front_kernel, dim3(plvs::ceil_div(n_pairs(), 256)), dim3(256), 0, stream, dtab, FP, fronts);
      PLVS_KERNEL_CHECK();
      ++launches;
      hipLaunchKernelGGL(fuse_window_kernel<true>, dim3(plvs::ceil_div(n_pairs(), 4)), dim3(256), 0, stream, dev, dtab, FP, th, fronts, rec);
    } else {
      hipLaunchKernelGGL(fuse_window_kernel<false>, dim3(plvs::ceil_div(n_pairs(), 4)), dim3(256), 0, stream, dev, dtab, FP, th, nullptr, rec);
    }
    return PLVS_OK;
  }

  void host_at(int k) override {
    grids.clear();
    grids.emplace_back(&kfs[k].view);
    tab.assign(1, KfDev{kf_const(kfs[k])});
  }
  fp::Result host_pair(int k, int i) override {
    const size_t at = device ? (size_t)k : 0;
    const plvs_fuse_keyframe& kf = kfs[k];
    return pair_host({grids[at].start.data(), grids[at].members.data(), kf.view.u_right, kf.view.desc, kf.view.scale_factors, kf.inv_level_sigma2},
                     tab[at].k, i);
  }
};

// ---------------------------------------------------------------------------------------------------- resident key frames
// Key frames resident in HBM (keyframe_handle.hpp): a KfRes table — pose, constants, pointers into the handles' allocations — and
// nothing else.  Nothing of a key frame is built, staged or copied.
struct ResidentPoints : PointPart {
  const plvs_keyframe* const* const kfs;
  const plvs_keyframe_pose* const poses;          // the SE3 search's
  const plvs_keyframe_sim3_pose* const sim3;      // the Sim3 search's (one of the two is null)
  const int layout;                               // of the Sim3 search
  std::vector<KfConst> consts;   // per listed key frame: the handle's constants with the call's pose

  ResidentPoints(const plvs_keyframe* const* kfs_, const plvs_keyframe_pose* poses_, const plvs_keyframe_sim3_pose* sim3_, int n_kfs_,
                 const plvs_fuse_points* P_, const uint8_t* skip_, float th_, const Outputs& out_, int32_t* stats_)
      : PointPart(n_kfs_, P_, skip_, th_, out_, stats_, 4), kfs(kfs_), poses(poses_), sim3(sim3_), layout(g_loop_layout) {
    if (sim3) gate = fp::kGateSim3;
  }

  bool has_points(int k) const override { return kfs[k]->pt.n > 0; }
  size_t table_entry() const override { return sizeof(KfRes); }

  void prepare_host() override {
    consts.resize((size_t)n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
      KfConst& c = consts[k] = kfs[k]->pt.c;
      for (int i = 0; i < 4; ++i) c.q[i] = sim3 ? sim3[k].q_cw[i] : poses[k].q_cw[i];
      for (int i = 0; i < 3; ++i) {
        c.t[i] = sim3 ? sim3[k].tcw[i] : poses[k].tcw[i];
        c.Ow[i] = sim3 ? sim3[k].Ow_points[i] : poses[k].Ow[i];
      }
    }
  }

  void fill_kfs(char* p) override {
    KfRes* tab = reinterpret_cast<KfRes*>(p + o_tab);
    for (int k = 0; k < n_kfs; ++k) tab[k] = KfRes{consts[k], arrays_at(kfs[k]->dev, kfs[k]->pt)};
  }

  int launch_kfs(char*, const char* table, const FusePoints& FP, int2* rec, hipStream_t stream) override {
    const KfRes* tab = reinterpret_cast<const KfRes*>(table);
    const dim3 per_pair(plvs::ceil_div(n_pairs(), 4));
    if (!sim3) {
      hipLaunchKernelGGL(fuse_window_resident_kernel<fp::kGateSE3>, per_pair, dim3(256), 0, stream, tab, FP, th, rec);
    } else if (layout == 1) {
      hipLaunchKernelGGL(fuse_window_resident_kernel<fp::kGateSim3>, per_pair, dim3(256), 0, stream, tab, FP, th, rec);
    } else {
      const int tiles = (int)plvs::ceil_div((size_t)P->m, 256);
      hipLaunchKernelGGL(loop_fuse_sieve_kernel, dim3((unsigned)n_kfs * (unsigned)tiles), dim3(256), 0, stream, tab, FP, th, tiles, rec);
    }
    return PLVS_OK;
  }

  fp::Result host_pair(int k, int i) override {   // on the handle's host copy
    const KfArrays a = arrays_at(kfs[k]->host.data(), kfs[k]->pt);
    return pair_host({a.start, a.members, a.u_right, reinterpret_cast<const uint8_t*>(a.desc), a.sf, a.sig}, consts[k], i);
  }
};

}  // namespace

int plvs::kfhandle::check_point_keyframe(const plvs_fuse_keyframe& kf, bool need_pose) {
  PLVS_REQUIRE(kf.n_cameras == 1 && kf.camera_model == PLVS_CAMERA_PINHOLE,
               "single-camera pinhole key frames only (NLeft == -1, bRight == false): the fisheye / two-camera branches stay with the reference");
  PLVS_REQUIRE(kf.K4 && kf.bounds4 && (!need_pose || (kf.q_cw && kf.tcw && kf.Ow)), "null pose / camera array");
  PLVS_REQUIRE(kf.n_levels >= 1 && kf.n_levels <= kMaxLevels && kf.inv_level_sigma2 && kf.view.scale_factors, "levels outside [1, 64] or null level arrays");
  PLVS_REQUIRE(kf.view.n >= 0 && kf.view.n < (1 << kPosBits), "key point count outside [0, 2^23)");
  if (kf.view.n > 0) {
    PLVS_REQUIRE(kf.view.x && kf.view.y && kf.view.octave && kf.view.u_right && kf.view.desc, "null key frame array");
    for (int i = 0; i < kf.view.n; ++i)
      PLVS_REQUIRE(kf.view.octave[i] >= 0 && kf.view.octave[i] < kf.n_levels, "octave of a key point outside the key frame's levels");
  }
  return PLVS_OK;
}

void plvs::kfhandle::stage_points(const plvs_fuse_keyframe& kf, plvs_keyframe* h) {
  plvs_keyframe::Points& s = h->pt;
  const FrameGrid grid(&kf.view);
  const size_t n = (size_t)kf.view.n;
  s.present = true;
  s.c = kf_const(kf, false);
  s.n = kf.view.n;
  s.n_levels = kf.n_levels;
  s.o_mem = put(&h->host, grid.members.data(), sizeof(FrameGrid::Member) * n);
  s.o_start = put(&h->host, grid.start.data(), sizeof(int) * grid.start.size());
  s.o_ur = put(&h->host, kf.view.u_right, sizeof(float) * n);
  s.o_desc = put(&h->host, kf.view.desc, n * 32);
  s.o_sf = put(&h->host, kf.view.scale_factors, sizeof(float) * (size_t)kf.n_levels);
  s.o_sig = put(&h->host, kf.inv_level_sigma2, sizeof(float) * (size_t)kf.n_levels);
}

int plvs::fusejob::make_point_part_kf(const plvs_keyframe* const* kfs, const plvs_keyframe_pose* poses, int n_kfs, const plvs_fuse_points* P,
                                      const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats,
                                      bool host_entry, std::unique_ptr<Part>* out, const plvs_keyframe_sim3_pose* sim3) {
  out->reset();
  int rc = check_call(kfs, n_kfs, P, th, best_idx, best_dist);
  if (rc == PLVS_OK) rc = check_handles(kfs, sim3 ? static_cast<const void*>(sim3) : poses, n_kfs, 1, host_entry);
  if (rc != PLVS_OK) return rc;
  if (n_kfs > 0 && P->m > 0) out->reset(new ResidentPoints(kfs, poses, sim3, n_kfs, P, skip, th, Outputs{best_idx, best_dist, reached}, stats));
  return PLVS_OK;
}

int plvs::fusejob::make_point_part(const plvs_fuse_keyframe* kfs, int n_kfs, const plvs_fuse_points* P, const uint8_t* skip, float th,
                                   int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats, std::unique_ptr<Part>* out) {
  out->reset();
  int rc = check_call(kfs, n_kfs, P, th, best_idx, best_dist);
  for (int k = 0; rc == PLVS_OK && k < n_kfs; ++k) rc = plvs::kfhandle::check_point_keyframe(kfs[k], true);
  if (rc != PLVS_OK) return rc;
  if (n_kfs > 0 && P->m > 0) out->reset(new StagedPoints(kfs, n_kfs, P, skip, th, Outputs{best_idx, best_dist, reached}, stats));
  return PLVS_OK;
}

extern "C" {

int plvs_hip_orb_fuse_search(const plvs_fuse_keyframe* kfs, int n_kfs, const plvs_fuse_points* P, const uint8_t* skip, float th,
                             int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats, void* stream) {
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_point_part(kfs, n_kfs, P, skip, th, best_idx, best_dist, reached, stats, &part);
  return rc != PLVS_OK ? rc : fj::run_single(part.get(), stats, 3, stream, false, g_chained == 2);
}

int plvs_hip_orb_fuse_search_host(const plvs_fuse_keyframe* kfs, int n_kfs, const plvs_fuse_points* P, const uint8_t* skip, float th,
                                  int32_t* best_idx, int32_t* best_dist, uint8_t* reached, int32_t* stats) {
  std::unique_ptr<fj::Part> part;
  const int rc = fj::make_point_part(kfs, n_kfs, P, skip, th, best_idx, best_dist, reached, stats, &part);
  return rc != PLVS_OK ? rc : fj::run_single(part.get(), stats, 3, nullptr, true);
}

void plvs_hip_orb_fuse_test_chained(int mode) { g_chained = (mode == 1 || mode == 2) ? mode : 0; }

void plvs_hip_loop_fuse_test_layout(int mode) { g_loop_layout = mode == 1 ? 1 : 0; }

}  // extern "C"
