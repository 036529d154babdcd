// brotli_copy_kernels.hip -- one launch that copies n independent byte segments of any alignment and any length (gfx950, wave64).
//
// The stream set (brotli_capi.cpp: BrotliAmdStreamSetDecompress) moves the chunks of many streaming states with it: one transfer brings all
// chunks to the device packed back to back, this kernel appends each to its state's input buffer; the other way round it gathers every state's
// new output into one staging buffer that one transfer brings back.  The neighbours of a segment in such a buffer are other states' bytes.
//
// Work is split by BYTES, not by segments: the segment walk of csrc/brotli_seg_walk.h over the words of DESTINATION memory, in tiles of
// BROTLI_AMD_COPY_TILE_BYTES.  A tile that lies inside one segment -- every tile of a long one -- is searched for once, not per lane.
//
// A unit is one aligned 16-byte store where the segment covers the whole word.  The first and last unit of a segment are EDGES: the bytes of
// the word that belong to the segment are stored as aligned dwords and single bytes, never as a read-modify-write of something wider -- what
// lies next to them is not this segment's.  The source of a unit is shifted against it by (src - dst) mod 16: the lane loads the one or two
// ALIGNED 16-byte words of source that hold the unit's bytes and shifts them together in registers.  A word is loaded only where it holds a
// byte of [src, src + len), so no load leaves the 16-byte-aligned span around the segment.
#include <hip/hip_runtime.h>

#include "brotli_device_abi.h"
#include "brotli_seg_walk.h"

namespace {

constexpr uint32_t kThreads = BROTLI_AMD_SEG_THREADS, kChunkSegs = BROTLI_AMD_SEG_CHUNK_SEGS;
constexpr uint32_t kUnitsPerThread = 4;
constexpr uint32_t kTileUnits = kThreads * kUnitsPerThread;

static_assert(kTileUnits * 16u == BROTLI_AMD_COPY_TILE_BYTES, "the tile the header names");

// bytes [s, s + 16) of the 32 bytes a : b (s in 0..15)
__host__ __device__ __forceinline__ BrotliAmdV4 shift_bytes(BrotliAmdV4 a, BrotliAmdV4 b, uint32_t s) {
  uint32_t t0, t1, t2, t3, t4;
  switch (s >> 2) {
    case 0: t0 = a.x; t1 = a.y; t2 = a.z; t3 = a.w; t4 = b.x; break;
    case 1: t0 = a.y; t1 = a.z; t2 = a.w; t3 = b.x; t4 = b.y; break;
    case 2: t0 = a.z; t1 = a.w; t2 = b.x; t3 = b.y; t4 = b.z; break;
    default: t0 = a.w; t1 = b.x; t2 = b.y; t3 = b.z; t4 = b.w; break;
  }
  const uint32_t sh = (s & 3u) * 8u;
  BrotliAmdV4 v;
  v.x = (uint32_t)((((uint64_t)t1 << 32) | t0) >> sh);
  v.y = (uint32_t)((((uint64_t)t2 << 32) | t1) >> sh);
  v.z = (uint32_t)((((uint64_t)t3 << 32) | t2) >> sh);
  v.w = (uint32_t)((((uint64_t)t4 << 32) | t3) >> sh);
  return v;
}

// unit k of a segment: the k-th aligned 16-byte word of destination memory that [dst, dst + len) touches
__host__ __device__ __forceinline__ void copy_unit(uint64_t src, uint64_t dst, uint64_t len, uint64_t k) {
  const uint64_t W = (dst & ~(uint64_t)15) + 16u * k;
  const uint64_t lo = W > dst ? W : dst, hi = W + 16u < dst + len ? W + 16u : dst + len;
  const uint64_t S = src + (W - dst);            // the source address of the word's byte 0 (below src in a first unit that starts inside its word)
  const uint32_t s = (uint32_t)S & 15u;
  const uint64_t SA = S - s;
  const uint64_t need_lo = S + (lo - W), need_hi = S + (hi - W);   // source bytes wanted: inside [src, src + len)
  BrotliAmdV4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
  if (need_lo < SA + 16u) a = *(const BROTLI_AMD_GLOBAL BrotliAmdV4*)SA;
  if (s != 0u && SA + 16u < need_hi) b = *(const BROTLI_AMD_GLOBAL BrotliAmdV4*)(SA + 16u);
  const BrotliAmdV4 v = shift_bytes(a, b, s);
  if (lo == W && hi == W + 16u) *(BROTLI_AMD_GLOBAL BrotliAmdV4*)W = v;
  else brotli_amd_seg_store_edge(W, lo, hi, v);
}

__global__ __launch_bounds__(kThreads) void brotli_amd_ragged_copy_kernel(const BrotliAmdCopySeg* __restrict__ segs, uint32_t n) {
  __shared__ uint64_t pre[kChunkSegs + 1];   // units in front of each segment of the chunk (in front of the chunk included); [kChunkSegs]: behind its last
  __shared__ uint64_t scan[kThreads];
  const uint32_t tid = threadIdx.x;
  brotli_amd_seg_walk<kTileUnits>(segs, n, pre, scan, [](const BrotliAmdCopySeg& sg) { return sg.dst; },
                                  [&](const uint64_t* pre, const BrotliAmdCopySeg* segs, uint32_t, uint64_t lo, uint64_t hi, uint64_t t0, uint64_t) {
    const uint32_t ja = brotli_amd_seg_find(pre, kChunkSegs, lo), jb = brotli_amd_seg_find(pre, kChunkSegs, hi - 1u);
    if (ja == jb) {   // one segment's: the rule for a long one
      const BrotliAmdCopySeg sg = segs[ja];
      const uint64_t first = pre[ja];
#pragma unroll
      for (uint32_t it = 0; it < kUnitsPerThread; it++) {
        const uint64_t g = t0 + it * kThreads + tid;
        if (g >= lo && g < hi) copy_unit((uint64_t)(uintptr_t)sg.src, (uint64_t)(uintptr_t)sg.dst, sg.len, g - first);
      }
    } else {
#pragma unroll
      for (uint32_t it = 0; it < kUnitsPerThread; it++) {
        const uint64_t g = t0 + it * kThreads + tid;
        if (g >= lo && g < hi) {
          const uint32_t j = brotli_amd_seg_find(pre, kChunkSegs, g);
          const BrotliAmdCopySeg sg = segs[j];
          copy_unit((uint64_t)(uintptr_t)sg.src, (uint64_t)(uintptr_t)sg.dst, sg.len, g - pre[j]);
        }
      }
    }
  });
}

}  // namespace

extern "C" uint32_t brotli_amd_copy_tile_bytes(void) { return BROTLI_AMD_COPY_TILE_BYTES; }

// max_bytes: what the segments' lengths add up to at most where the caller knows (0: unknown) -- a launch of a few short segments then has a
// few blocks, not a device full of blocks that find nothing to do
extern "C" hipError_t brotli_amd_launch_ragged_copy_sized(const BrotliAmdCopySeg* d_segs, uint32_t n, uint64_t max_bytes, hipStream_t stream) {
  if (n == 0u) return hipSuccess;
  uint32_t grid = 0;
  // (a segment touches at most len / 16 + 2 words)
  const hipError_t e = brotli_amd_seg_grid(max_bytes != 0u ? max_bytes / 16u + 2u * (uint64_t)n : 0u, kTileUnits, &grid);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(brotli_amd_ragged_copy_kernel, dim3(grid), dim3(kThreads), 0, stream, d_segs, n);
  return hipGetLastError();
}

extern "C" hipError_t brotli_amd_launch_ragged_copy(const BrotliAmdCopySeg* d_segs, uint32_t n, hipStream_t stream) {
  return brotli_amd_launch_ragged_copy_sized(d_segs, n, 0u, stream);
}
