// The runtime half of the CUDA stand-in (cuda_runtime.h says what it promises): fibers, the block scheduler, the
// rendezvous of barriers and shuffles, and a filling allocator.  Written from scratch; one host thread only.
#include "cuda_runtime.h"

#include <sys/mman.h>

#include <vector>

#if !defined(__x86_64__)
#include <ucontext.h>
#endif

uint3 threadIdx, blockIdx;
dim3 blockDim, gridDim;

namespace {

int g_fill = 0;
unsigned long g_undefined_shuffles = 0;

// ---------------------------------------------------------------- context switch
// x86-64: a hand-written switch of the callee-saved registers (swapcontext costs a signal-mask system call per
// switch, and a pair of images makes millions of them).  Elsewhere: ucontext.
#if defined(__x86_64__)
extern "C" void cuda_shim_switch(void** save_sp, void* load_sp) __attribute__((visibility("hidden")));
asm(R"(
        .text
        .hidden cuda_shim_switch
        .globl  cuda_shim_switch
        .type   cuda_shim_switch, @function
cuda_shim_switch:
        pushq %rbp
        pushq %rbx
        pushq %r12
        pushq %r13
        pushq %r14
        pushq %r15
        movq  %rsp, (%rdi)
        movq  %rsi, %rsp
        popq  %r15
        popq  %r14
        popq  %r13
        popq  %r12
        popq  %rbx
        popq  %rbp
        ret
        .size cuda_shim_switch, .-cuda_shim_switch
)");
typedef void* Context;
#else
typedef ucontext_t Context;
#endif

enum State { READY, AT_BARRIER, AT_SYNCWARP, AT_SHFL, DONE };

struct Fiber {
  Context ctx;
  char* stack = nullptr;
  State state = DONE;
  uint3 tid;
  unsigned lane = 0, warp = 0;
  // what it waits with
  int kind = 0, width = 0;
  unsigned mask = 0, arg = 0;
  uint64_t bits = 0;
};

const size_t kStack = 256 * 1024;   // mapped lazily; kernels keep a few hundred bytes of locals
std::vector<Fiber> g_fibers;        // grown to the largest block seen, stacks reused
Context g_main;
Fiber* g_cur = nullptr;
unsigned g_n = 0;                   // threads of the running block
unsigned g_live = 0, g_at_barrier = 0;
const char* g_kernel = "";
void (*g_thread_fn)(void*) = nullptr;
void* g_thread_ctx = nullptr;

[[noreturn]] void die(const char* what, const Fiber* f) {
  fprintf(stderr, "cuda_shim: %s — kernel %s, block (%u, %u), thread (%u, %u, %u) = warp %u lane %u\n", what, g_kernel,
          blockIdx.x, blockIdx.y, f ? f->tid.x : 0, f ? f->tid.y : 0, f ? f->tid.z : 0, f ? f->warp : 0, f ? f->lane : 0);
  fflush(stderr);
  abort();
}

void to_main(Fiber* f) {
#if defined(__x86_64__)
  cuda_shim_switch(&f->ctx, g_main);
#else
  swapcontext(&f->ctx, &g_main);
#endif
}

void to_fiber(Fiber* f) {
  g_cur = f;
  threadIdx = f->tid;
#if defined(__x86_64__)
  cuda_shim_switch(&g_main, f->ctx);
#else
  swapcontext(&g_main, &f->ctx);
#endif
  g_cur = nullptr;
}

void fiber_entry() {
  Fiber* f = g_cur;
  g_thread_fn(g_thread_ctx);
  f->state = DONE;
  to_main(f);
  die("a finished thread was resumed", f);
}

void prepare(Fiber* f) {
  if (!f->stack) {
    void* p = mmap(nullptr, kStack, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (p == MAP_FAILED) die("no memory for a thread's stack", nullptr);
    f->stack = static_cast<char*>(p);
  }
#if defined(__x86_64__)
  // on entry of a function rsp is 8 below a multiple of 16; six registers and the entry address lie under that
  void** top = reinterpret_cast<void**>((reinterpret_cast<uintptr_t>(f->stack + kStack) & ~uintptr_t(15)) - 8);
  *top = nullptr;                                   // the return address fiber_entry never uses
  *(top - 1) = reinterpret_cast<void*>(&fiber_entry);
  for (int i = 2; i <= 7; ++i) *(top - i) = nullptr;
  f->ctx = top - 7;
#else
  getcontext(&f->ctx);
  f->ctx.uc_stack.ss_sp = f->stack;
  f->ctx.uc_stack.ss_size = kStack;
  f->ctx.uc_link = nullptr;
  makecontext(&f->ctx, fiber_entry, 0);
#endif
}

// ---------------------------------------------------------------- rendezvous
Fiber& lane_of(unsigned warp, unsigned lane) { return g_fibers[warp * 32 + lane]; }
bool lane_exists(unsigned warp, unsigned lane) { return warp * 32 + lane < g_n; }

// all live lanes of `mask` in this warp wait in `state` with the same mask -> true
bool group_complete(const Fiber& f, State state) {
  for (unsigned l = 0; l < 32; ++l) {
    if (!(f.mask >> l & 1) || !lane_exists(f.warp, l)) continue;
    const Fiber& o = lane_of(f.warp, l);
    if (o.state == DONE) continue;
    if (o.state != state || o.mask != f.mask) return false;
    if (state == AT_SHFL && (o.kind != f.kind || o.width != f.width)) return false;
  }
  return true;
}

// CUDA's source-lane table; -1: the lane keeps its own value
int source_lane(int kind, unsigned lane, unsigned arg, int width) {
  const unsigned seg = lane & ~(unsigned)(width - 1), last = seg + width - 1;
  switch (kind) {
    case cuda_shim::SHFL_IDX: return (int)(seg | (arg & (unsigned)(width - 1)));
    case cuda_shim::SHFL_UP: return (lane < arg || lane - arg < seg) ? -1 : (int)(lane - arg);
    case cuda_shim::SHFL_DOWN: return (arg > 31 || lane + arg > last) ? -1 : (int)(lane + arg);
    default: { const unsigned j = lane ^ arg; return j > last ? -1 : (int)j; }   // an earlier segment may be read
  }
}

void release_shfl(const Fiber& f) {
  uint64_t result[32];
  for (unsigned l = 0; l < 32; ++l) {
    if (!(f.mask >> l & 1) || !lane_exists(f.warp, l)) continue;
    Fiber& o = lane_of(f.warp, l);
    if (o.state != AT_SHFL) continue;
    const int src = source_lane(o.kind, l, o.arg, o.width);
    if (src < 0) { result[l] = o.bits; continue; }
    if (!(f.mask >> src & 1)) {            // undefined in CUDA: the fill pattern, and counted
      ++g_undefined_shuffles;
      result[l] = 0x0101010101010101ull * (uint64_t)(g_fill & 0xff);
      continue;
    }
    if (!lane_exists(f.warp, (unsigned)src) || lane_of(f.warp, (unsigned)src).state != AT_SHFL)
      die("a shuffle reads from a lane of its mask that has left the kernel", &o);
    result[l] = lane_of(f.warp, (unsigned)src).bits;
  }
  for (unsigned l = 0; l < 32; ++l) {
    if (!(f.mask >> l & 1) || !lane_exists(f.warp, l)) continue;
    Fiber& o = lane_of(f.warp, l);
    if (o.state != AT_SHFL) continue;
    o.bits = result[l];
    o.state = READY;
  }
}

void release_syncwarp(const Fiber& f) {
  for (unsigned l = 0; l < 32; ++l)
    if ((f.mask >> l & 1) && lane_exists(f.warp, l) && lane_of(f.warp, l).state == AT_SYNCWARP) lane_of(f.warp, l).state = READY;
}

// after a thread stopped running (it waits, or it is done): whatever that completes is released
void settle(Fiber& f) {
  if (f.state == AT_SHFL) { if (group_complete(f, AT_SHFL)) release_shfl(f); }
  else if (f.state == AT_SYNCWARP) { if (group_complete(f, AT_SYNCWARP)) release_syncwarp(f); }
  if (f.state == DONE) {   // its leaving may complete what the others of its warp wait for
    for (unsigned l = 0; l < 32; ++l) {
      if (!lane_exists(f.warp, l)) continue;
      Fiber& o = lane_of(f.warp, l);
      if (o.state == AT_SHFL && group_complete(o, AT_SHFL)) release_shfl(o);
      else if (o.state == AT_SYNCWARP && group_complete(o, AT_SYNCWARP)) release_syncwarp(o);
    }
  }
  if (f.state == AT_BARRIER) ++g_at_barrier;
  if (f.state == DONE) --g_live;
  if (g_at_barrier && g_at_barrier == g_live) {   // __syncthreads: the block's live threads
    for (unsigned t = 0; t < g_n; ++t)
      if (g_fibers[t].state == AT_BARRIER) g_fibers[t].state = READY;
    g_at_barrier = 0;
  }
}

void wait_as(State s) {
  Fiber* f = g_cur;
  if (!f) die("a device synchronisation was called outside a kernel", nullptr);
  f->state = s;
  to_main(f);
}

void run_block() {
  for (unsigned t = 0; t < g_n; ++t) {
    Fiber& f = g_fibers[t];
    f.tid.x = t % blockDim.x;
    f.tid.y = t / blockDim.x % blockDim.y;
    f.tid.z = t / (blockDim.x * blockDim.y);
    f.warp = t / 32;
    f.lane = t % 32;
    f.state = READY;
    prepare(&f);
  }
  g_live = g_n;
  g_at_barrier = 0;
  for (;;) {
    bool ran = false;
    unsigned live = 0;
    for (unsigned t = 0; t < g_n; ++t) {
      Fiber& f = g_fibers[t];
      if (f.state == READY) {
        to_fiber(&f);
        settle(f);
        ran = true;
      }
      live += f.state != DONE;
    }
    if (!live) return;
    if (!ran) {   // everybody waits and nothing can complete: in CUDA a hang or an undefined result
      for (unsigned t = 0; t < g_n; ++t)
        if (g_fibers[t].state == AT_SHFL) die("a shuffle waits for a lane of its mask that is not at the same shuffle", &g_fibers[t]);
      for (unsigned t = 0; t < g_n; ++t)
        if (g_fibers[t].state != DONE) die("a barrier waits for threads that never arrive", &g_fibers[t]);
    }
  }
}

}  // namespace

namespace cuda_shim {

void run_grid(const char* kernel, const LaunchCfg& c, void (*thread_fn)(void*), void* ctx) {
  if (g_cur) die("a launch from inside a kernel", g_cur);
  const size_t n = (size_t)c.block.x * c.block.y * c.block.z;
  if (n == 0 || n > 1024 || c.grid.x == 0 || c.grid.y == 0 || c.grid.z == 0) {
    fprintf(stderr, "cuda_shim: invalid launch configuration of %s: grid (%u, %u, %u), block (%u, %u, %u)\n", kernel, c.grid.x,
            c.grid.y, c.grid.z, c.block.x, c.block.y, c.block.z);
    if (n == 0 || n > 1024) abort();
    return;   // an empty grid: CUDA reports cudaErrorInvalidConfiguration and runs nothing
  }
  if (g_fibers.size() < n) g_fibers.resize(n);
  g_kernel = kernel;
  g_thread_fn = thread_fn;
  g_thread_ctx = ctx;
  g_n = (unsigned)n;
  blockDim = c.block;
  gridDim = c.grid;
  for (unsigned z = 0; z < c.grid.z; ++z)
    for (unsigned y = 0; y < c.grid.y; ++y)
      for (unsigned x = 0; x < c.grid.x; ++x) {
        blockIdx.x = x;
        blockIdx.y = y;
        blockIdx.z = z;
        run_block();
      }
  g_kernel = "";
}

uint64_t shfl(int kind, unsigned mask, uint64_t bits, unsigned arg, int width) {
  Fiber* f = g_cur;
  if (!f) die("a shuffle was called outside a kernel", nullptr);
  if (width < 1 || width > 32 || (width & (width - 1))) die("a shuffle's width is no power of two up to 32", f);
  if (!(mask >> f->lane & 1)) die("a shuffle's mask does not name the calling lane", f);
  f->kind = kind;
  f->mask = mask;
  f->bits = bits;
  f->arg = arg;
  f->width = width;
  wait_as(AT_SHFL);
  return f->bits;
}

void syncthreads() { wait_as(AT_BARRIER); }

void syncwarp(unsigned mask) {
  Fiber* f = g_cur;
  if (!f) die("__syncwarp was called outside a kernel", nullptr);
  if (!(mask >> f->lane & 1)) die("__syncwarp's mask does not name the calling lane", f);
  f->mask = mask;
  wait_as(AT_SYNCWARP);
}

}  // namespace cuda_shim

// ---------------------------------------------------------------- runtime calls
static cudaError_t alloc_filled(void** p, size_t bytes, int fill) {
  if (!p) return cudaErrorInvalidValue;
  void* q = nullptr;
  if (posix_memalign(&q, 256, bytes ? bytes : 1) != 0) { *p = nullptr; return cudaErrorMemoryAllocation; }
  memset(q, fill, bytes);
  *p = q;
  return cudaSuccess;
}
cudaError_t cudaMalloc(void** p, size_t bytes) { return alloc_filled(p, bytes, g_fill); }
cudaError_t cuda_shim_malloc_zero(void** p, size_t bytes) { return alloc_filled(p, bytes, 0); }
cudaError_t cudaFree(void* p) { free(p); return cudaSuccess; }
cudaError_t cudaMemset(void* p, int value, size_t bytes) { memset(p, value, bytes); return cudaSuccess; }
cudaError_t cudaMemcpy(void* dst, const void* src, size_t bytes, cudaMemcpyKind) { memmove(dst, src, bytes); return cudaSuccess; }
cudaError_t cudaGetLastError() { return cudaSuccess; }
const char* cudaGetErrorString(cudaError_t e) {
  return e == cudaSuccess ? "no error" : e == cudaErrorMemoryAllocation ? "out of memory" : "invalid value";
}

extern "C" {
void cuda_shim_set_fill(int byte) { g_fill = byte & 0xff; }
unsigned long cuda_shim_undefined_shuffles() { return g_undefined_shuffles; }
void cuda_shim_reset_counters() { g_undefined_shuffles = 0; }
}
