// brotli_copy_kernels.hip -- one launch that copies n independent byte segments of any alignment and any length (gfx950, wave64).
//
// The stream set (brotli_capi.cpp: BrotliAmdStreamSetDecompress) moves the chunks of many streaming states with it: one transfer brings all
// chunks to the device packed back to back, this kernel appends each to its state's input buffer; the other way round it gathers every state's
// new output into one staging buffer that one transfer brings back.  The neighbours of a segment in such a buffer are other states' bytes.
//
// Work is split by BYTES, not by segments.  A segment's UNITS are the 16-byte-aligned words of destination memory it touches; the units of all
// segments, one after the other, are cut into tiles of kTileUnits (BROTLI_AMD_COPY_TILE_BYTES of destination), and the blocks take the tiles
// in turns.  One long segment among a thousand short ones is spread over every block, and a thousand short ones are a dozen tiles.  A lane
// finds the segment of a unit by a binary search in the prefix sum of the segments' unit counts, which every block builds in LDS for
// kChunkSegs segments at a time (the launch gets the segment table alone, so no block knows beforehand where its tiles lie); a tile that lies
// inside one segment -- every tile of a long one -- is searched for once, not per lane.
//
// A unit is one aligned 16-byte store where the segment covers the whole word.  The first and last unit of a segment are EDGES: the bytes of
// the word that belong to the segment are stored as aligned dwords and single bytes, never as a read-modify-write of something wider -- what
// lies next to them is not this segment's.  The source of a unit is shifted against it by (src - dst) mod 16: the lane loads the one or two
// ALIGNED 16-byte words of source that hold the unit's bytes and shifts them together in registers.  A word is loaded only where it holds a
// byte of [src, src + len), so no load leaves the 16-byte-aligned span around the segment.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "brotli_device_abi.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kUnitsPerThread = 4;
constexpr uint32_t kTileUnits = kThreads * kUnitsPerThread;
constexpr uint32_t kChunkSegs = kThreads * 4;   // segments whose prefix sum lies in LDS at a time: four a thread
// (global-memory instructions, not flat ones: the addresses are computed as integers, so the address space is said where they are used)
#if defined(__HIP_DEVICE_COMPILE__)
#define BROTLI_AMD_GLOBAL __attribute__((address_space(1)))
#else
#define BROTLI_AMD_GLOBAL
#endif
typedef uint32_t v4u __attribute__((ext_vector_type(4)));   // sixteen bytes a lane

static_assert(kTileUnits * 16u == BROTLI_AMD_COPY_TILE_BYTES, "the tile the header names");

__host__ __device__ __forceinline__ uint64_t seg_units(uint64_t dst, uint64_t len) { return len ? ((dst + len + 15u) >> 4) - (dst >> 4) : 0u; }

// bytes [s, s + 16) of the 32 bytes a : b (s in 0..15)
__host__ __device__ __forceinline__ v4u shift_bytes(v4u a, v4u b, uint32_t s) {
  uint32_t t0, t1, t2, t3, t4;
  switch (s >> 2) {
    case 0: t0 = a.x; t1 = a.y; t2 = a.z; t3 = a.w; t4 = b.x; break;
    case 1: t0 = a.y; t1 = a.z; t2 = a.w; t3 = b.x; t4 = b.y; break;
    case 2: t0 = a.z; t1 = a.w; t2 = b.x; t3 = b.y; t4 = b.z; break;
    default: t0 = a.w; t1 = b.x; t2 = b.y; t3 = b.z; t4 = b.w; break;
  }
  const uint32_t sh = (s & 3u) * 8u;
  v4u v;
  v.x = (uint32_t)((((uint64_t)t1 << 32) | t0) >> sh);
  v.y = (uint32_t)((((uint64_t)t2 << 32) | t1) >> sh);
  v.z = (uint32_t)((((uint64_t)t3 << 32) | t2) >> sh);
  v.w = (uint32_t)((((uint64_t)t4 << 32) | t3) >> sh);
  return v;
}

// bytes [lo, hi) of the word at W (lo, hi inside [W, W + 16], not the whole word): aligned dwords where the segment has all four bytes, single bytes elsewhere
__host__ __device__ __forceinline__ void store_edge(uint64_t W, uint64_t lo, uint64_t hi, v4u v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (uint32_t i = 0; i < 4u; i++) {
    const uint64_t A = W + 4u * i;
    if (A >= lo && A + 4u <= hi) { *(BROTLI_AMD_GLOBAL uint32_t*)A = w[i]; continue; }
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++)
      if (A + j >= lo && A + j < hi) *(BROTLI_AMD_GLOBAL uint8_t*)(A + j) = (uint8_t)(w[i] >> (8u * j));
  }
}

// unit k of a segment: the k-th aligned 16-byte word of destination memory that [dst, dst + len) touches
__host__ __device__ __forceinline__ void copy_unit(uint64_t src, uint64_t dst, uint64_t len, uint64_t k) {
  const uint64_t W = (dst & ~(uint64_t)15) + 16u * k;
  const uint64_t lo = W > dst ? W : dst, hi = W + 16u < dst + len ? W + 16u : dst + len;
  const uint64_t S = src + (W - dst);            // the source address of the word's byte 0 (below src in a first unit that starts inside its word)
  const uint32_t s = (uint32_t)S & 15u;
  const uint64_t SA = S - s;
  const uint64_t need_lo = S + (lo - W), need_hi = S + (hi - W);   // source bytes wanted: inside [src, src + len)
  v4u a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
  if (need_lo < SA + 16u) a = *(const BROTLI_AMD_GLOBAL v4u*)SA;
  if (s != 0u && SA + 16u < need_hi) b = *(const BROTLI_AMD_GLOBAL v4u*)(SA + 16u);
  const v4u v = shift_bytes(a, b, s);
  if (lo == W && hi == W + 16u) *(BROTLI_AMD_GLOBAL v4u*)W = v;
  else store_edge(W, lo, hi, v);
}

// the segment of unit g: pre[j] <= g < pre[j + 1] (pre[0] <= g < pre[kChunkSegs]; a segment without units is never the answer)
__host__ __device__ __forceinline__ uint32_t find_seg(const uint64_t* pre, uint64_t g) {
  uint32_t a = 0, b = kChunkSegs;
  while (b - a > 1u) { const uint32_t m = (a + b) >> 1; if (pre[m] <= g) a = m; else b = m; }
  return a;
}

// This block's tiles among the units [base, end) of one chunk of segments (pre[]: the units in front of each, segs: the chunk's first): every thread
// of the block makes the same walk and copies its own units.  -> the block's next tile (one that goes on behind `end` stays the block's).
__host__ __device__ __forceinline__ uint64_t take_tiles(const uint64_t* pre, const BrotliAmdCopySeg* segs, uint64_t base, uint64_t end, uint64_t tile,
                                                        uint32_t grid, uint32_t tid) {
  while (tile * kTileUnits < end) {
    const uint64_t t0 = tile * kTileUnits, t1 = t0 + kTileUnits;
    const uint64_t lo = t0 > base ? t0 : base, hi = t1 < end ? t1 : end;   // the tile's units among this chunk's segments
    if (lo < hi) {   // (not: a tile that began in the chunk before, and this chunk has no units)
      const uint32_t ja = find_seg(pre, lo), jb = find_seg(pre, hi - 1u);
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
            const uint32_t j = find_seg(pre, g);
            const BrotliAmdCopySeg sg = segs[j];
            copy_unit((uint64_t)(uintptr_t)sg.src, (uint64_t)(uintptr_t)sg.dst, sg.len, g - pre[j]);
          }
        }
      }
    }
    if (t1 > end) break;   // (the tile goes on in the next chunk's segments)
    tile += grid;
  }
  return tile;
}

__global__ __launch_bounds__(kThreads) void brotli_amd_ragged_copy_kernel(const BrotliAmdCopySeg* __restrict__ segs, uint32_t n) {
  __shared__ uint64_t pre[kChunkSegs + 1];   // units in front of each segment of the chunk (in front of the chunk included); [kChunkSegs]: behind its last
  __shared__ uint64_t scan[kThreads];
  const uint32_t tid = threadIdx.x;
  uint64_t base = 0;              // units of the segments in front of the chunk
  uint64_t tile = blockIdx.x;     // this block's next tile
  for (uint32_t c0 = 0; c0 < n; c0 += kChunkSegs) {
    const uint32_t cnt = n - c0 < kChunkSegs ? n - c0 : kChunkSegs;
    uint64_t u[4], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
      const uint32_t j = 4u * tid + k;
      u[k] = j < cnt ? seg_units((uint64_t)(uintptr_t)segs[c0 + j].dst, segs[c0 + j].len) : 0u;
      sum += u[k];
    }
    __syncthreads();   // (the chunk before is done with pre[])
    scan[tid] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < kThreads; off <<= 1) {
      const uint64_t v = tid >= off ? scan[tid - off] : 0u;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    uint64_t at = base + scan[tid] - sum;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) { pre[4u * tid + k] = at; at += u[k]; }
    const uint64_t end = base + scan[kThreads - 1u];
    if (tid == 0u) pre[kChunkSegs] = end;
    __syncthreads();
    tile = take_tiles(pre, segs + c0, base, end, tile, gridDim.x, tid);
    base = end;
  }
}

}  // namespace

extern "C" uint32_t brotli_amd_copy_tile_bytes(void) { return BROTLI_AMD_COPY_TILE_BYTES; }

// max_bytes: what the segments' lengths add up to at most where the caller knows (0: unknown) -- a launch of a few short segments then has a
// few blocks, not a device full of blocks that find nothing to do
extern "C" hipError_t brotli_amd_launch_ragged_copy_sized(const BrotliAmdCopySeg* d_segs, uint32_t n, uint64_t max_bytes, hipStream_t stream) {
  if (n == 0u) return hipSuccess;
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  uint64_t grid = (uint64_t)(cus > 0 ? cus : 1) * 4u;   // four blocks of four waves a CU
  if (max_bytes != 0u) {
    const uint64_t units = max_bytes / 16u + 2u * (uint64_t)n;   // (a segment touches at most len / 16 + 2 words)
    grid = std::min<uint64_t>(grid, (units + kTileUnits - 1u) / kTileUnits);
  }
  hipLaunchKernelGGL(brotli_amd_ragged_copy_kernel, dim3((uint32_t)grid), dim3(kThreads), 0, stream, d_segs, n);
  return hipGetLastError();
}

extern "C" hipError_t brotli_amd_launch_ragged_copy(const BrotliAmdCopySeg* d_segs, uint32_t n, hipStream_t stream) {
  return brotli_amd_launch_ragged_copy_sized(d_segs, n, 0u, stream);
}
