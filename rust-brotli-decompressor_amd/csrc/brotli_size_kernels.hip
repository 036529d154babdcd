// brotli_size_kernels.hip -- the size walk (csrc/brotli_size_walk.h) over the streams of a batch in one launch (gfx950, wave64).
//
// ONE LANE PER STREAM.  A walk is a short chain of dependent loads -- a header says where the next one lies --, so a stream has no
// parallelism of its own to give a wave; the width is across the streams of the batch.  Blocks of 256 threads take the streams in a
// grid-stride loop.  A lane's bit window is one ALIGNED dword of its stream, loaded anew when the walk asks for a byte outside it: the walk
// asks for bytes of [in, in + in_size) alone, so every dword loaded holds at least one of them, whatever the alignment of `in`, and an
// aligned dword never leaves the page of a byte it holds.  The payloads of stored and metadata metablocks are stepped over by arithmetic.
// The kernel writes hints[i], and nothing else.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "brotli_size_walk.h"

namespace {

constexpr uint32_t kThreads = 256;

// byte i of a stream through the aligned dword that holds it
struct DwordWindow {
  uint64_t base;                 // address of byte 0
  uint64_t have = ~(uint64_t)0;  // address of the dword in `word` (none yet)
  uint32_t word = 0;
  __device__ uint32_t operator()(uint64_t i) {
    const uint64_t a = base + i, aligned = a & ~(uint64_t)3;
    if (aligned != have) { word = *reinterpret_cast<const uint32_t*>(aligned); have = aligned; }
    return (word >> (8u * (uint32_t)(a & 3u))) & 0xFFu;
  }
};

__global__ __launch_bounds__(kThreads) void brotli_amd_size_walk_kernel(const BrotliAmdSizeDesc* __restrict__ descs, uint32_t n, uint32_t flags,
                                                                        BrotliAmdSizeHint* __restrict__ hints) {
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    const BrotliAmdSizeDesc d = descs[i];
    DwordWindow w;
    w.base = (uint64_t)(uintptr_t)d.in;
    hints[i] = brotli_amd_size_walk(w, d.in_size, flags);
  }
}

}  // namespace

extern "C" hipError_t brotli_amd_launch_size_walk(const BrotliAmdSizeDesc* d_descs, uint32_t n, uint32_t flags, BrotliAmdSizeHint* d_hints,
                                                  hipStream_t stream) {
  if (n == 0u) return hipSuccess;
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  // at most four blocks a CU (sixteen waves: enough walks in flight to hide their loads): beyond that the grid-stride loop takes the rest
  const uint32_t grid = std::min<uint32_t>((n + kThreads - 1u) / kThreads, (uint32_t)(cus > 0 ? cus : 1) * 4u);
  hipLaunchKernelGGL(brotli_amd_size_walk_kernel, dim3(grid), dim3(kThreads), 0, stream, d_descs, n, flags, d_hints);
  return hipGetLastError();
}
