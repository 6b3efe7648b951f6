// Host-side Delaunay triangulation of libelas' support points: the observable behaviour of
// Elas::computeDelaunayTriangulation (Thirdparty/libelas-gpu/CPU/elas.cpp:492-556), which hands the points to Shewchuk's
// Triangle as triangulate("zQB") (CPU/triangle.cpp).  The support points sit on a 5-px grid, so the triangulation is not
// unique, and computeDisparity rasterises the triangles in order: the map depends on which diagonal the program picks,
// on the order of its triangles and on the order of each one's corners.  This file reproduces all three.
//
// What "zQB" runs (no -p, no refinement, no -l): the divide-and-conquer construction with alternating cuts
// (divconqdelaunay, triangle.cpp:6162-6230), on a random seed reset by every call (triangleinit, :4032):
//   1. the vertices are quicksorted by (x, y) with random pivots drawn from a linear congruential generator
//      (vertexsort :5448-5501, randomnation :4049-4050);
//   2. of equal vertices the first in sorted order survives, with its input index (:6181-6197): which one that is depends
//      on the pivots, hence the same generator and the same partition scheme here;
//   3. the array is reordered for alternating cuts by median splits on x or y (alternateaxes / vertexmedian
//      :5513-5603; they draw from the same generator, reproduced as well although the resulting sets do not depend on it);
//   4. the halves are triangulated recursively (divconqrecurse :5955-6105; leaves of 2 and 3 vertices, three collinear
//      ones included) and knitted together along their lower common tangent (mergehulls :5640-5953), every choice under
//      exact `ccw > 0`, `ccw <= 0` and `incircle > 0` tests;
//   5. the bounding ("ghost") triangles of the hull are deleted (removeghosts :6107-6160) and the survivors are written
//      in allocation order, each as (org, dest, apex) of its orientation 0 (writeelements :7802-7860).
// Triangles are only ever created in this path, and a bounding triangle the merge turns into a real one keeps its slot,
// so the output order is the order of creation.  The predicates are exact integer arithmetic here: the coordinates are
// integers (u, v, u - d, width - 1 + d) and the reference's adaptive predicates are exact as well, so the signs agree.
// Coordinates must stay below 2^24 in magnitude (the reference stores them as float).
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace plvs {
namespace elas_dt {

// Triangle-based mesh: every triangle has three corners (vertex index or -1 = none yet) and three links, one across each
// of its edges.  An oriented triangle `Side` names one edge: its apex is corner[o], the edge runs from corner[o + 1] to
// corner[o + 2] (mod 3), and link[o] holds the oriented triangle on the other side as 3 * triangle + orientation.
// Triangle 0 is the "outside" every unlinked edge points to.
struct Side {
  int t, o;
  bool operator==(const Side& s) const { return t == s.t && o == s.o; }
};

class Triangulator {
 public:
  // xs / ys: n vertex coordinates.  Appends every output triangle's (org, dest, apex) input indices to `corners`.
  void run(const int32_t* xs, const int32_t* ys, int n, std::vector<int32_t>& corners) {
    x_ = xs;
    y_ = ys;
    seed_ = 1;
    corner_.assign(3, -1);
    link_.assign(3, 0);
    corners.clear();
    if (n < 3) return;
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    sort_xy(order.data(), n);
    int m = 0;                                             // duplicates: the first in sorted order stays
    for (int j = 1; j < n; ++j)
      if (x_[order[m]] != x_[order[j]] || y_[order[m]] != y_[order[j]]) order[++m] = order[j];
    ++m;
    if (m < 3) return;                                     // one edge at most: only bounding triangles
    const int half = m >> 1;
    if (m - half >= 2) {
      if (half >= 2) alternate(order.data(), half, 1);
      alternate(order.data() + half, m - half, 1);
    }
    Side hull_l, hull_r;
    build(order.data(), m, 0, hull_l, hull_r);
    // the bounding triangles around the hull are the ones with a corner left empty (the ring removeghosts walks and
    // deletes); the rest, in the order they were made
    const int nt = (int)corner_.size() / 3;
    for (int t = 1; t < nt; ++t) {
      const int32_t* c = &corner_[3 * t];
      if (c[0] < 0 || c[1] < 0 || c[2] < 0) continue;
      corners.push_back(c[1]);
      corners.push_back(c[2]);
      corners.push_back(c[0]);
    }
  }

 private:
  const int32_t* x_ = nullptr;
  const int32_t* y_ = nullptr;
  uint64_t seed_ = 1;
  std::vector<int32_t> corner_, link_;

  // ------------------------------------------------ the generator and the two partitions (triangle.cpp:4049-4050, 5448-5603)
  unsigned draw(unsigned choices) {
    seed_ = (seed_ * 1366u + 150889u) % 714025u;
    return (unsigned)(seed_ / (714025u / choices + 1u));
  }
  int64_t coord(int v, int axis) const { return axis ? y_[v] : x_[v]; }
  // a sorts before b on (axis, other axis)
  bool before(int a, int b, int axis) const {
    return coord(a, axis) < coord(b, axis) || (coord(a, axis) == coord(b, axis) && coord(a, 1 - axis) < coord(b, 1 - axis));
  }
  // Hoare-style split around a random pivot: afterwards [0, lo) sorts before or equal the pivot, (hi, n) after or equal
  void split(int* a, int n, int axis, int& lo, int& hi) {
    const int p = a[draw((unsigned)n)];
    lo = -1;
    hi = n;
    while (lo < hi) {
      do ++lo; while (lo <= hi && before(a[lo], p, axis));
      do --hi; while (lo <= hi && before(p, a[hi], axis));
      if (lo < hi) std::swap(a[lo], a[hi]);
    }
  }
  void sort_xy(int* a, int n) {
    if (n == 2) {
      if (before(a[1], a[0], 0)) std::swap(a[0], a[1]);
      return;
    }
    int lo, hi;
    split(a, n, 0, lo, hi);
    if (lo > 1) sort_xy(a, lo);
    if (hi < n - 2) sort_xy(a + hi + 1, n - hi - 1);
  }
  // the first k of a[0, n) end up before the others on (axis, other axis)
  void select(int* a, int n, int k, int axis) {
    if (n == 2) {
      if (before(a[1], a[0], axis)) std::swap(a[0], a[1]);
      return;
    }
    int lo, hi;
    split(a, n, axis, lo, hi);
    if (lo > k) select(a, lo, k, axis);
    if (hi < k - 1) select(a + hi + 1, n - hi - 1, k - hi - 1, axis);
  }
  void alternate(int* a, int n, int axis) {
    const int half = n >> 1;
    if (n <= 3) axis = 0;                                  // the leaves are always sorted by x
    select(a, n, half, axis);
    if (n - half >= 2) {
      if (half >= 2) alternate(a, half, 1 - axis);
      alternate(a + half, n - half, 1 - axis);
    }
  }

  // ------------------------------------------------ exact predicates
  // > 0: a, b, c counterclockwise
  int64_t ccw(int a, int b, int c) const {
    return ((int64_t)x_[a] - x_[c]) * ((int64_t)y_[b] - y_[c]) - ((int64_t)y_[a] - y_[c]) * ((int64_t)x_[b] - x_[c]);
  }
  // sign of the incircle determinant: > 0 when d lies inside the circle through a, b, c (counterclockwise)
  int incircle(int a, int b, int c, int d) const {
    const int64_t ax = (int64_t)x_[a] - x_[d], ay = (int64_t)y_[a] - y_[d];
    const int64_t bx = (int64_t)x_[b] - x_[d], by = (int64_t)y_[b] - y_[d];
    const int64_t cx = (int64_t)x_[c] - x_[d], cy = (int64_t)y_[c] - y_[d];
    const __int128 det = (__int128)(ax * ax + ay * ay) * (bx * cy - cx * by) + (__int128)(bx * bx + by * by) * (cx * ay - ax * cy) +
                         (__int128)(cx * cx + cy * cy) * (ax * by - bx * ay);
    return det > 0 ? 1 : (det < 0 ? -1 : 0);
  }

  // ------------------------------------------------ mesh primitives
  static Side next(Side s) { return {s.t, s.o == 2 ? 0 : s.o + 1}; }
  static Side prev(Side s) { return {s.t, s.o == 0 ? 2 : s.o - 1}; }
  Side across(Side s) const {
    const int e = link_[3 * s.t + s.o];
    return {e / 3, e % 3};
  }
  int org(Side s) const { return corner_[3 * s.t + (s.o == 2 ? 0 : s.o + 1)]; }
  int dst(Side s) const { return corner_[3 * s.t + (s.o == 0 ? 2 : s.o - 1)]; }
  int apx(Side s) const { return corner_[3 * s.t + s.o]; }
  void set_org(Side s, int v) { corner_[3 * s.t + (s.o == 2 ? 0 : s.o + 1)] = v; }
  void set_dst(Side s, int v) { corner_[3 * s.t + (s.o == 0 ? 2 : s.o - 1)] = v; }
  void set_apx(Side s, int v) { corner_[3 * s.t + s.o] = v; }
  void glue(Side a, Side b) {
    link_[3 * a.t + a.o] = 3 * b.t + b.o;
    link_[3 * b.t + b.o] = 3 * a.t + a.o;
  }
  Side fresh() {
    const int t = (int)corner_.size() / 3;
    corner_.insert(corner_.end(), {-1, -1, -1});
    link_.insert(link_.end(), {0, 0, 0});
    return {t, 0};
  }

  // ------------------------------------------------ divide and conquer (divconqrecurse, triangle.cpp:5955-6105)
  // On return: org(left_end) is the leftmost vertex, dst(right_end) the rightmost (both bounding triangles).
  void build(const int* a, int n, int axis, Side& left_end, Side& right_end) {
    if (n == 2) {                                          // an edge: two bounding triangles back to back
      left_end = fresh();
      set_org(left_end, a[0]);
      set_dst(left_end, a[1]);
      right_end = fresh();
      set_org(right_end, a[1]);
      set_dst(right_end, a[0]);
      for (int k = 0; k < 3; ++k) {
        glue(left_end, right_end);
        if (k == 2) break;
        left_end = prev(left_end);
        right_end = next(right_end);
      }
      left_end = prev(right_end);
      return;
    }
    if (n == 3) {                                          // a triangle and three bounding ones, or two edges
      Side core = fresh(), g1 = fresh(), g2 = fresh(), g3 = fresh();
      const int64_t area = ccw(a[0], a[1], a[2]);
      if (area == 0) {
        set_org(core, a[0]);
        set_dst(core, a[1]);
        set_org(g1, a[1]);
        set_dst(g1, a[0]);
        set_org(g2, a[2]);
        set_dst(g2, a[1]);
        set_org(g3, a[1]);
        set_dst(g3, a[2]);
        for (int k = 0; k < 3; ++k) {
          if (k == 1) {
            glue(core, g3);
            glue(g1, g2);
          } else {
            glue(core, g1);
            glue(g2, g3);
          }
          if (k < 2) {
            core = next(core);
            g1 = prev(g1);
            g2 = next(g2);
            g3 = prev(g3);
          }
        }
        left_end = g1;
        right_end = g2;
        return;
      }
      const int second = area > 0 ? a[1] : a[2], third = area > 0 ? a[2] : a[1];
      set_org(core, a[0]);
      set_dst(g1, a[0]);
      set_org(g3, a[0]);
      set_dst(core, second);
      set_org(g1, second);
      set_dst(g2, second);
      set_apx(core, third);
      set_org(g2, third);
      set_dst(g3, third);
      glue(core, g1);
      core = next(core);
      glue(core, g2);
      core = next(core);
      glue(core, g3);
      g1 = prev(g1);
      g2 = next(g2);
      glue(g1, g2);
      g1 = prev(g1);
      g3 = prev(g3);
      glue(g1, g3);
      g2 = next(g2);
      g3 = prev(g3);
      glue(g2, g3);
      left_end = g1;
      right_end = area > 0 ? g2 : next(left_end);
      return;
    }
    const int half = n >> 1;
    Side inner_l, inner_r;
    build(a, half, 1 - axis, left_end, inner_l);
    build(a + half, n - half, 1 - axis, inner_r, right_end);
    merge(left_end, inner_l, inner_r, right_end, axis);
  }

  // ------------------------------------------------ knitting two triangulations (mergehulls, triangle.cpp:5640-5953)
  // far_l / inner_l: bounding triangles of the left part (org(far_l) leftmost, dst(inner_l) rightmost vertex); inner_r /
  // far_r: of the right part (org(inner_r) leftmost, dst(far_r) rightmost).  axis 1: the parts lie below / above each other.
  void merge(Side& far_l, Side& inner_l, Side& inner_r, Side& far_r, int axis) {
    int il_dst = dst(inner_l), il_apx = apx(inner_l);
    int ir_org = org(inner_r), ir_apx = apx(inner_r);
    if (axis == 1) {
      // move the four handles from the leftmost / rightmost to the bottommost / topmost vertices
      int fl_pt = org(far_l), fl_apx = apx(far_l);
      while (y_[fl_apx] < y_[fl_pt]) {
        far_l = across(next(far_l));
        fl_pt = fl_apx;
        fl_apx = apx(far_l);
      }
      Side probe = across(inner_l);
      int pv = apx(probe);
      while (y_[pv] > y_[il_dst]) {
        inner_l = next(probe);
        il_apx = il_dst;
        il_dst = pv;
        probe = across(inner_l);
        pv = apx(probe);
      }
      while (y_[ir_apx] < y_[ir_org]) {
        inner_r = across(next(inner_r));
        ir_org = ir_apx;
        ir_apx = apx(inner_r);
      }
      int fr_pt = dst(far_r);
      probe = across(far_r);
      pv = apx(probe);
      while (y_[pv] > y_[fr_pt]) {
        far_r = next(probe);
        fr_pt = pv;
        probe = across(far_r);
        pv = apx(probe);
      }
    }
    // the lower common tangent
    for (bool moved = true; moved;) {
      moved = false;
      if (ccw(il_dst, il_apx, ir_org) > 0) {
        inner_l = across(prev(inner_l));
        il_dst = il_apx;
        il_apx = apx(inner_l);
        moved = true;
      }
      if (ccw(ir_apx, ir_org, il_dst) > 0) {
        inner_r = across(next(inner_r));
        ir_org = ir_apx;
        ir_apx = apx(inner_r);
        moved = true;
      }
    }
    Side cand_l = across(inner_l), cand_r = across(inner_r);
    Side base = fresh();                                   // the new bounding triangle below the seam
    glue(base, inner_l);
    base = next(base);
    glue(base, inner_r);
    base = next(base);
    set_org(base, ir_org);
    set_dst(base, il_dst);
    if (il_dst == org(far_l)) far_l = next(base);
    if (ir_org == dst(far_r)) far_r = prev(base);
    int low_l = il_dst, low_r = ir_org;
    int up_l = apx(cand_l), up_r = apx(cand_r);
    for (;;) {
      const bool done_l = ccw(up_l, low_l, low_r) <= 0, done_r = ccw(up_r, low_l, low_r) <= 0;
      if (done_l && done_r) {
        Side top = fresh();                                // the new bounding triangle above the seam
        set_org(top, low_l);
        set_dst(top, low_r);
        glue(top, base);
        top = next(top);
        glue(top, cand_r);
        top = next(top);
        glue(top, cand_l);
        if (axis == 1) {
          // the handles back to the leftmost / rightmost vertices
          int fl_pt = org(far_l), fr_pt = dst(far_r), fr_apx = apx(far_r);
          Side probe = across(far_l);
          int pv = apx(probe);
          while (x_[pv] < x_[fl_pt]) {
            far_l = prev(probe);
            fl_pt = pv;
            probe = across(far_l);
            pv = apx(probe);
          }
          while (x_[fr_apx] > x_[fr_pt]) {
            far_r = across(prev(far_r));
            fr_pt = fr_apx;
            fr_apx = apx(far_r);
          }
        }
        return;
      }
      if (!done_l) {                                       // flip away left edges that fail the circle test
        Side nx = across(prev(cand_l));
        int nv = apx(nx);
        bool bad = nv >= 0 && incircle(low_l, low_r, up_l, nv) > 0;
        while (bad) {
          nx = next(nx);
          const Side top_c = across(nx);
          nx = next(nx);
          const Side side_c = across(nx);
          glue(nx, top_c);
          glue(cand_l, side_c);
          cand_l = next(cand_l);
          const Side outer_c = across(cand_l);
          nx = prev(nx);
          glue(nx, outer_c);
          set_org(cand_l, low_l);
          set_dst(cand_l, -1);
          set_apx(cand_l, nv);
          set_org(nx, -1);
          set_dst(nx, up_l);
          set_apx(nx, nv);
          up_l = nv;
          nx = side_c;
          nv = apx(nx);
          bad = nv >= 0 && incircle(low_l, low_r, up_l, nv) > 0;
        }
      }
      if (!done_r) {                                       // the same on the right
        Side nx = across(next(cand_r));
        int nv = apx(nx);
        bool bad = nv >= 0 && incircle(low_l, low_r, up_r, nv) > 0;
        while (bad) {
          nx = prev(nx);
          const Side top_c = across(nx);
          nx = prev(nx);
          const Side side_c = across(nx);
          glue(nx, top_c);
          glue(cand_r, side_c);
          cand_r = prev(cand_r);
          const Side outer_c = across(cand_r);
          nx = next(nx);
          glue(nx, outer_c);
          set_org(cand_r, -1);
          set_dst(cand_r, low_r);
          set_apx(cand_r, nv);
          set_org(nx, up_r);
          set_dst(nx, -1);
          set_apx(nx, nv);
          up_r = nv;
          nx = side_c;
          nv = apx(nx);
          bad = nv >= 0 && incircle(low_l, low_r, up_r, nv) > 0;
        }
      }
      if (done_l || (!done_r && incircle(up_l, low_l, low_r, up_r) > 0)) {
        glue(base, cand_r);                                // new edge low_l - up_r
        base = prev(cand_r);
        set_dst(base, low_l);
        low_r = up_r;
        cand_r = across(base);
        up_r = apx(cand_r);
      } else {
        glue(base, cand_l);                                // new edge up_l - low_r
        base = next(cand_l);
        set_org(base, low_r);
        low_l = up_l;
        cand_l = across(base);
        up_l = apx(cand_l);
      }
    }
  }
};

}  // namespace elas_dt
}  // namespace plvs
