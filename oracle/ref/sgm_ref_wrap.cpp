// C interface of oracle/_ref/libsgm_ref.so: libsgm's own CUDA sources (Thirdparty/libsgm/src), compiled for the CPU
// against the stand-in of cuda_shim/ and executed by it.  This file is ours; everything it calls is the reference's:
//   sgm_ref_execute  the whole sgm::StereoSGM(w, h, 64, 8, 8, EXECUTE_INOUT_HOST2HOST, Parameters(P1, P2, uniqueness))
//                    ::execute, as PointCloudKeyFrame::ProcessStereoLibsgm constructs and calls it
//   sgm_ref_stages   the same chain stage by stage through the classes the reference's headers declare
//                    (CensusTransform, PathAggregation<64>, WinnerTakesAll<64>) and median_filter / check_consistency of
//                    internal.h, with the buffers allocated and cleared as CudaStereoSGMResources does
//                    (stereo_sgm.cpp: cudaMalloc + cudaMemset(0) of the four disparity images)
#include <libsgm.h>

#include "census_transform.hpp"
#include "internal.h"
#include "path_aggregation.hpp"
#include "winner_takes_all.hpp"

extern "C" {

void sgm_ref_set_fill(int byte) { cuda_shim_set_fill(byte); }
unsigned long sgm_ref_undefined_shuffles() { return cuda_shim_undefined_shuffles(); }
void sgm_ref_reset_counters() { cuda_shim_reset_counters(); }

void sgm_ref_execute(const uint8_t* left, const uint8_t* right, int w, int h, int p1, int p2, float uniqueness, uint8_t* out) {
  sgm::StereoSGM sgm(w, h, 64, 8, 8, sgm::EXECUTE_INOUT_HOST2HOST, sgm::StereoSGM::Parameters(p1, p2, uniqueness));
  sgm.execute(left, right, out);
}

// census_*: w*h u32; paths: 8 volumes of w*h*64 u8 in PathAggregation::get_output()'s order; the rest w*h u8
void sgm_ref_stages(const uint8_t* left, const uint8_t* right, int w, int h, int p1, int p2, float uniqueness,
                    uint32_t* census_left, uint32_t* census_right, uint8_t* paths, uint8_t* raw_left, uint8_t* raw_right,
                    uint8_t* median_left, uint8_t* median_right, uint8_t* final_left) {
  const size_t n = (size_t)w * h;
  uint8_t *d_left, *d_right, *d_disp_l, *d_disp_r, *d_tmp_l, *d_tmp_r;
  CudaSafeCall(cudaMalloc(&d_left, n));
  CudaSafeCall(cudaMalloc(&d_right, n));
  uint8_t** disp[] = {&d_disp_l, &d_disp_r, &d_tmp_l, &d_tmp_r};
  for (uint8_t** p : disp) {
    CudaSafeCall(cudaMalloc(p, sizeof(uint16_t) * n));
    CudaSafeCall(cudaMemset(*p, 0, sizeof(uint16_t) * n));
  }
  CudaSafeCall(cudaMemcpy(d_left, left, n, cudaMemcpyHostToDevice));
  CudaSafeCall(cudaMemcpy(d_right, right, n, cudaMemcpyHostToDevice));
  {
    sgm::CensusTransform<uint8_t> cl, cr;
    sgm::PathAggregation<64> pa;
    sgm::WinnerTakesAll<64> wta;
    cl.enqueue(d_left, w, h, 0);
    cr.enqueue(d_right, w, h, 0);
    pa.enqueue(cl.get_output(), cr.get_output(), w, h, (unsigned)p1, (unsigned)p2, 0);
    wta.enqueue(d_tmp_l, d_tmp_r, pa.get_output(), w, h, uniqueness, 0);
    CudaSafeCall(cudaMemcpy(census_left, cl.get_output(), n * 4, cudaMemcpyDeviceToHost));
    CudaSafeCall(cudaMemcpy(census_right, cr.get_output(), n * 4, cudaMemcpyDeviceToHost));
    CudaSafeCall(cudaMemcpy(paths, pa.get_output(), n * 64 * 8, cudaMemcpyDeviceToHost));
  }
  CudaSafeCall(cudaMemcpy(raw_left, d_tmp_l, n, cudaMemcpyDeviceToHost));
  CudaSafeCall(cudaMemcpy(raw_right, d_tmp_r, n, cudaMemcpyDeviceToHost));
  sgm::details::median_filter(d_tmp_l, d_disp_l, w, h);
  sgm::details::median_filter(d_tmp_r, d_disp_r, w, h);
  CudaSafeCall(cudaMemcpy(median_left, d_disp_l, n, cudaMemcpyDeviceToHost));
  CudaSafeCall(cudaMemcpy(median_right, d_disp_r, n, cudaMemcpyDeviceToHost));
  sgm::details::check_consistency(d_disp_l, d_disp_r, d_left, w, h, 8);
  CudaSafeCall(cudaMemcpy(final_left, d_disp_l, n, cudaMemcpyDeviceToHost));
  void* bufs[] = {d_left, d_right, d_disp_l, d_disp_r, d_tmp_l, d_tmp_r};
  for (void* b : bufs) CudaSafeCall(cudaFree(b));
}

}  // extern "C"
