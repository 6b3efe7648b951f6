// A stand-in for the CUDA runtime and device language, written from scratch: it lets g++ compile libsgm's .cu sources
// as they lie and EXECUTES a launch on the host with CUDA's semantics (oracle/ref/Makefile: libsgm_ref.so).  Test
// infrastructure only; the runtime half is cuda_shim.cpp.
//
// Execution model
//   * A launch runs its blocks one after another on the calling host thread.  The threads of a block are
//     cooperatively scheduled fibers; each fiber sees its own threadIdx (set when it is switched in), while blockIdx,
//     blockDim and gridDim are the block's.
//   * `__shared__` becomes STATIC storage.  That is valid only because exactly one block exists at a time and
//     everything runs on one host thread: never call into this library from two threads.
//   * __syncthreads is a rendezvous of the block's live threads (threads that returned do not take part);
//     __syncwarp(mask) one of the live lanes of `mask` in a warp of 32.
//   * __shfl_*_sync(mask, var, x, width) is a rendezvous of the live lanes of `mask`; the source lane follows CUDA's
//     table (programming guide, "Warp Shuffle Functions"): segments of `width` lanes, a lane keeps its own value where
//     up / down / xor would leave its segment upwards (xor may reach into an EARLIER segment).
//       - source lane inside `mask` but returned from the kernel, or never arriving at the same shuffle: the process
//         stops with a message naming the kernel and the lane (no made-up value);
//       - source lane outside `mask`: CUDA leaves the value undefined.  libsgm does this at every subgroup edge
//         (path_aggregation_common.hpp: __shfl_up_sync(mask-of-a-subgroup, ., 1) with the default width 32) and discards
//         the result.  The shim returns the allocation fill byte replicated, so a result that depended on it would
//         differ between the two fills the pinned test runs, and counts them (cuda_shim_undefined_shuffles).
//   * cudaMalloc fills what it returns with cuda_shim_set_fill()'s byte: an answer that depends on memory the
//     sources never wrote is visible, not lucky.  Streams and events do nothing: every call is synchronous.
//   * kernel<<<grid, block, shmem, stream>>>(args) is not C++: launch_rewrite.sed turns that expression, and nothing
//     else, into cuda_shim::launch("kernel", cuda_shim::cfg(grid, block, shmem, stream), <call of kernel>)(args).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static

// Vector types.  No over-alignment on purpose: the sources load them through reinterpret_cast from addresses CUDA
// guarantees aligned but the host's static arrays need not be.
struct uchar2 { unsigned char x, y; };
struct uchar4 { unsigned char x, y, z, w; };
struct ushort2 { unsigned short x, y; };
struct ushort4 { unsigned short x, y, z, w; };
struct uint2 { unsigned int x, y; };
struct uint3 { unsigned int x, y, z; };
struct uint4 { unsigned int x, y, z, w; };
struct dim3 {
  unsigned int x, y, z;
  dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};

extern uint3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;
static const int warpSize = 32;

// ---------------------------------------------------------------- runtime
enum cudaError { cudaSuccess = 0, cudaErrorMemoryAllocation = 2, cudaErrorInvalidValue = 1 };
typedef cudaError cudaError_t;
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice, cudaMemcpyDefault };
typedef struct cuda_shim_stream* cudaStream_t;
typedef struct cuda_shim_event* cudaEvent_t;

cudaError_t cudaMalloc(void** p, size_t bytes);
cudaError_t cuda_shim_malloc_zero(void** p, size_t bytes);   // for sgm_zero_malloc.h
template <class T> inline cudaError_t cudaMalloc(T** p, size_t bytes) { return cudaMalloc(reinterpret_cast<void**>(p), bytes); }
cudaError_t cudaFree(void* p);
cudaError_t cudaMemset(void* p, int value, size_t bytes);
cudaError_t cudaMemcpy(void* dst, const void* src, size_t bytes, cudaMemcpyKind kind);
cudaError_t cudaGetLastError();
const char* cudaGetErrorString(cudaError_t e);
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline cudaError_t cudaStreamCreate(cudaStream_t* s) { *s = nullptr; return cudaSuccess; }
inline cudaError_t cudaStreamDestroy(cudaStream_t) { return cudaSuccess; }
inline cudaError_t cudaStreamSynchronize(cudaStream_t) { return cudaSuccess; }
inline cudaError_t cudaStreamWaitEvent(cudaStream_t, cudaEvent_t, unsigned int) { return cudaSuccess; }
inline cudaError_t cudaEventCreate(cudaEvent_t* e) { *e = nullptr; return cudaSuccess; }
inline cudaError_t cudaEventDestroy(cudaEvent_t) { return cudaSuccess; }
inline cudaError_t cudaEventRecord(cudaEvent_t, cudaStream_t = nullptr) { return cudaSuccess; }
inline cudaError_t cudaEventSynchronize(cudaEvent_t) { return cudaSuccess; }

extern "C" {
void cuda_shim_set_fill(int byte);              // the byte cudaMalloc fills with (default 0)
unsigned long cuda_shim_undefined_shuffles();   // shuffles whose source lane lay outside the mask, since the last reset
void cuda_shim_reset_counters();
}

// ---------------------------------------------------------------- launches
namespace cuda_shim {
struct LaunchCfg { dim3 grid, block; };
inline LaunchCfg cfg(dim3 grid, dim3 block, size_t = 0, cudaStream_t = nullptr) { return LaunchCfg{grid, block}; }
void run_grid(const char* kernel, const LaunchCfg& c, void (*thread_fn)(void*), void* ctx);
template <class F> struct Launcher {
  const char* name;
  LaunchCfg c;
  F f;
  template <class... A> void operator()(A... a) {   // arguments are passed by value, as a launch does
    auto body = [&] { f(a...); };
    run_grid(name, c, [](void* p) { (*static_cast<decltype(body)*>(p))(); }, &body);
  }
};
template <class F> inline Launcher<F> launch(const char* name, LaunchCfg c, F f) { return Launcher<F>{name, c, f}; }

enum ShflKind { SHFL_IDX, SHFL_UP, SHFL_DOWN, SHFL_XOR };
uint64_t shfl(int kind, unsigned mask, uint64_t bits, unsigned arg, int width);
void syncthreads();
void syncwarp(unsigned mask);
template <class T> inline T shfl_t(int kind, unsigned mask, T var, unsigned arg, int width) {
  static_assert(sizeof(T) <= 8, "shuffles move 4- or 8-byte values");
  uint64_t b = 0;
  memcpy(&b, &var, sizeof(T));
  b = shfl(kind, mask, b, arg, width);
  memcpy(&var, &b, sizeof(T));
  return var;
}
}  // namespace cuda_shim

inline void __syncthreads() { cuda_shim::syncthreads(); }
inline void __syncwarp(unsigned mask = 0xffffffffu) { cuda_shim::syncwarp(mask); }
inline void __threadfence_block() {}
template <class T> inline T __shfl_sync(unsigned mask, T var, int src_lane, int width = warpSize) {
  return cuda_shim::shfl_t(cuda_shim::SHFL_IDX, mask, var, (unsigned)src_lane, width);
}
template <class T> inline T __shfl_up_sync(unsigned mask, T var, unsigned delta, int width = warpSize) {
  return cuda_shim::shfl_t(cuda_shim::SHFL_UP, mask, var, delta, width);
}
template <class T> inline T __shfl_down_sync(unsigned mask, T var, unsigned delta, int width = warpSize) {
  return cuda_shim::shfl_t(cuda_shim::SHFL_DOWN, mask, var, delta, width);
}
template <class T> inline T __shfl_xor_sync(unsigned mask, T var, int lane_mask, int width = warpSize) {
  return cuda_shim::shfl_t(cuda_shim::SHFL_XOR, mask, var, (unsigned)lane_mask, width);
}

// ---------------------------------------------------------------- device functions
template <class T> inline T __ldg(const T* p) { return *p; }
inline int __popc(unsigned int v) { return __builtin_popcount(v); }
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
inline unsigned int min(unsigned int a, unsigned int b) { return a < b ? a : b; }
inline unsigned int max(unsigned int a, unsigned int b) { return a > b ? a : b; }

// per-halfword / per-byte SIMD-in-a-word intrinsics: each lane of the word on its own
#define CUDA_SHIM_LANES(name, bits, expr)                                                   \
  inline unsigned int name(unsigned int a, unsigned int b) {                                \
    unsigned int r = 0;                                                                     \
    const unsigned int m = (bits == 8) ? 0xffu : 0xffffu;                                   \
    for (int s = 0; s < 32; s += bits) {                                                    \
      const unsigned int x = (a >> s) & m, y = (b >> s) & m;                                \
      r |= ((unsigned int)(expr) & m) << s;                                                 \
    }                                                                                       \
    return r;                                                                               \
  }
CUDA_SHIM_LANES(__vcmpgtu2, 16, x > y ? m : 0u)
CUDA_SHIM_LANES(__vcmpgtu4, 8, x > y ? m : 0u)
CUDA_SHIM_LANES(__vminu2, 16, x < y ? x : y)
CUDA_SHIM_LANES(__vminu4, 8, x < y ? x : y)
CUDA_SHIM_LANES(__vmaxu2, 16, x > y ? x : y)
CUDA_SHIM_LANES(__vmaxu4, 8, x > y ? x : y)
#undef CUDA_SHIM_LANES
