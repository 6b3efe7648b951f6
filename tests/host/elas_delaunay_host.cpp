// Host compile of the product's support-point triangulation (plvs_amd/csrc/elas_delaunay.hpp) — the same file the
// library builds with hipcc — for CPU-side agreement checks under other compilers.  Test infrastructure only.
#include <cstdint>
#include <vector>

#include "../../plvs_amd/csrc/elas_delaunay.hpp"

// support: n x {u, v, d}; right_image: the points are (u - d, v).  Writes up to cap (c1, c2, c3) triples, returns the
// number of triangles.
extern "C" int hostdt_triangulate(const int32_t* support, int n, int right_image, int32_t* corners, int cap) {
  std::vector<int32_t> xs(n), ys(n), out;
  for (int i = 0; i < n; ++i) {
    xs[i] = right_image ? support[3 * i] - support[3 * i + 2] : support[3 * i];
    ys[i] = support[3 * i + 1];
  }
  plvs::elas_dt::Triangulator().run(xs.data(), ys.data(), n, out);
  const int nt = (int)out.size() / 3;
  for (int i = 0; i < 3 * nt && i < 3 * cap; ++i) corners[i] = out[i];
  return nt;
}
