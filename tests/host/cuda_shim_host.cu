// Test-only kernels for the CUDA stand-in of oracle/ref/cuda_shim/ (the thing that executes libsgm's kernels on the
// CPU for oracle/_ref/libsgm_ref.so): a wrong stand-in would pin the oracle to the stand-in's mistakes, so its
// shuffles, barriers, early exits and packed intrinsics are checked directly (tests/test_oracle_pinned_sgm.py).
// CUDA-style source of our own; the launches are rewritten by cuda_shim/launch_rewrite.sed like the reference's.
#include <cuda_runtime.h>

namespace {

// every lane offers lane + 100 * (warp + 1); out[thread] = what the shuffle returned
__global__ void shfl_kernel(unsigned* out, int kind, unsigned arg, int width) {
  const unsigned v = threadIdx.x % 32 + 100 * (threadIdx.x / 32 + 1);
  unsigned r = 0;
  if (kind == 0) r = __shfl_sync(0xffffffffu, v, (int)arg, width);
  if (kind == 1) r = __shfl_up_sync(0xffffffffu, v, arg, width);
  if (kind == 2) r = __shfl_down_sync(0xffffffffu, v, arg, width);
  if (kind == 3) r = __shfl_xor_sync(0xffffffffu, v, (int)arg, width);
  out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}

// two warps hand values to each other through shared memory, twice; block b offers other values than block b - 1,
// whose values still lie in the (static) array: without a working barrier a thread reads those
__global__ void exchange_kernel(unsigned* out) {
  __shared__ unsigned box[64];
  const unsigned t = threadIdx.x, base = 1000 * (blockIdx.x + 1);
  box[t] = base + t;
  __syncthreads();
  const unsigned got = box[(t + 32) % 64];
  __syncthreads();
  box[t] = 2 * got;
  __syncthreads();
  out[blockIdx.x * 64 + t] = box[(t + 33) % 64];
}

// 96 threads: warp 1 returns at once; in warp 0 the upper half returns before the lower half's shuffle and
// __syncwarp; warps 0 (lower half) and 2 then meet at a block barrier
__global__ void early_exit_kernel(unsigned* out) {
  __shared__ unsigned box[96];
  const unsigned t = threadIdx.x, lane = t % 32, warp = t / 32;
  out[t] = 7;
  if (warp == 1) return;
  if (warp == 0 && lane >= 16) return;
  unsigned v = t;
  if (warp == 0) {
    v = __shfl_down_sync(0x0000ffffu, t, 1, 16);    // lane 15 keeps its own
    __syncwarp(0x0000ffffu);
  }
  box[t] = v;
  __syncthreads();
  out[t] = box[warp == 0 ? 64 + lane : lane % 16] + 1;
}

// a lane of the mask has left: the stand-in must stop the process
__global__ void dead_lane_kernel(unsigned* out) {
  if (threadIdx.x == 3) return;
  out[threadIdx.x] = __shfl_sync(0xffffffffu, threadIdx.x, 3);
}

// the source lane lies outside the mask (libsgm does this at a subgroup's edge): the fill pattern comes back
__global__ void outside_mask_kernel(unsigned* out) {
  const unsigned group = threadIdx.x / 8;
  out[threadIdx.x] = __shfl_up_sync(0xffu << (8 * group), threadIdx.x + 1, 1);
}

__global__ void packed_kernel(const unsigned* a, const unsigned* b, unsigned* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[0 * n + i] = __vcmpgtu2(a[i], b[i]);
  out[1 * n + i] = __vcmpgtu4(a[i], b[i]);
  out[2 * n + i] = __vminu2(a[i], b[i]);
  out[3 * n + i] = __vminu4(a[i], b[i]);
  out[4 * n + i] = __vmaxu2(a[i], b[i]);
  out[5 * n + i] = __vmaxu4(a[i], b[i]);
}

template <class F> void with_device_words(unsigned* host, size_t n, F f) {
  unsigned* d;
  cudaMalloc(&d, n * 4);
  f(d);
  cudaMemcpy(host, d, n * 4, cudaMemcpyDeviceToHost);
  cudaFree(d);
}

}  // namespace

extern "C" {

void shimtest_shfl(unsigned* out, int kind, unsigned arg, int width) {   // out: 2 blocks of 64 threads
  with_device_words(out, 128, [&](unsigned* d) { shfl_kernel<<<2, 64>>>(d, kind, arg, width); });
}
void shimtest_exchange(unsigned* out) {   // out: 3 blocks of 64
  with_device_words(out, 192, [&](unsigned* d) { exchange_kernel<<<3, 64, 0, 0>>>(d); });
}
void shimtest_early_exit(unsigned* out) {   // out: 96
  with_device_words(out, 96, [&](unsigned* d) { early_exit_kernel<<<dim3(1), dim3(96)>>>(d); });
}
void shimtest_dead_lane(unsigned* out) {
  with_device_words(out, 32, [&](unsigned* d) { dead_lane_kernel<<<1, 32>>>(d); });
}
void shimtest_outside_mask(unsigned* out) {
  with_device_words(out, 32, [&](unsigned* d) { outside_mask_kernel<<<1, 32>>>(d); });
}
void shimtest_packed(const unsigned* a, const unsigned* b, unsigned* out, int n) {
  unsigned *da, *db;
  cudaMalloc(&da, (size_t)n * 4);
  cudaMalloc(&db, (size_t)n * 4);
  cudaMemcpy(da, a, (size_t)n * 4, cudaMemcpyHostToDevice);
  cudaMemcpy(db, b, (size_t)n * 4, cudaMemcpyHostToDevice);
  with_device_words(out, (size_t)n * 6, [&](unsigned* d) { packed_kernel << <(n + 127) / 128, 128 >> > (da, db, d, n); });
  cudaFree(da);
  cudaFree(db);
}
unsigned shimtest_malloc_byte(int fill) {   // what a fresh allocation holds
  cuda_shim_set_fill(fill);
  unsigned char* d;
  cudaMalloc(&d, 64);
  const unsigned v = d[0] | (unsigned)d[63] << 8;
  cudaFree(d);
  cuda_shim_set_fill(0);
  return v;
}

}  // extern "C"
