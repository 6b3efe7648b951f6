// Two more C entry points over the reference's open_chisel library, for scripts/make_chisel_scan_golden.py and
// scripts/make_chisel_scan_edges_golden.py only:
// Chisel::IntegrateDepthScanColorWithOneCameraModelBGR<float, uint8_t> on a handle of oracle/ref/chisel_full_ref_wrap.cpp
// (whose FullRef — chisel::Chisel + ProjectionIntegrator + PinholeCamera set up as ChiselServer does,
// ChiselServer.cpp:623-647 — and read-back entry points are taken as they are).  Compiled into a temporary directory
// against the reference's headers, oracle/ref/eigen_full and oracle/_ref/libchisel_full_ref.so; never shipped.
// It holds calls only.
#include "chisel_full_ref_wrap.cpp"

#include <open_chisel/camera/ColorImage.h>

extern "C" void ref_chisel_scan_integrate(void* p, const float* depth, const uint8_t* bgr, int channels, const float* Twc) {
  FullRef* h = static_cast<FullRef*>(p);
  const int w = h->camera.GetWidth(), hgt = h->camera.GetHeight();
  std::shared_ptr<chisel::DepthImage<float> > d(new chisel::DepthImage<float>(w, hgt));
  std::memcpy(d->GetMutableData(), depth, sizeof(float) * (size_t)w * hgt);
  std::shared_ptr<chisel::ColorImage<uint8_t> > c(new chisel::ColorImage<uint8_t>(w, hgt, (size_t)channels));
  std::memcpy(c->GetMutableData(), bgr, (size_t)w * hgt * channels);
  const std::shared_ptr<const chisel::DepthImage<float> > dc = d;
  const std::shared_ptr<const chisel::ColorImage<uint8_t> > cc = c;
  const chisel::Transform T = pose_of(Twc);
  h->map->IntegrateDepthScanColorWithOneCameraModelBGR<float, uint8_t>(h->integrator, dc, T, h->camera, cc, T, h->camera);
}

// For scripts/make_chisel_scan_edges_golden.py: another camera on the same map (the setters ref_chisel_full_create uses).
// (Seeded chunks go through ref_chisel_set_chunk of oracle/ref/chisel_set_chunk_ref_wrap.cpp: DistVoxel / ColorVoxel setters.)
extern "C" void ref_chisel_scan_set_camera(void* p, float fx, float fy, float cx, float cy, int width, int height,
                                           float near_plane, float far_plane) {
  FullRef* h = static_cast<FullRef*>(p);
  chisel::Intrinsics in;
  in.SetFx(fx); in.SetFy(fy); in.SetCx(cx); in.SetCy(cy);
  h->camera.SetIntrinsics(in);
  h->camera.SetWidth(width);
  h->camera.SetHeight(height);
  h->camera.SetNearPlane(near_plane);
  h->camera.SetFarPlane(far_plane);
  h->far_plane = far_plane;
}

