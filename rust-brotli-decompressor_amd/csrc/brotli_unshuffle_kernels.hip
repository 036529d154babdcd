// brotli_unshuffle_kernels.hip -- one launch that turns the byte planes of n independent segments, of any alignment, length and width
// (1, 2, 4, 8), back into elements (gfx950, wave64).  The transform, and what one unit of work reads and writes, is csrc/brotli_unshuffle.h.
//
// Work is split by BYTES, not by segments, the way csrc/brotli_copy_kernels.hip splits a copy (read the two side by side: the chunk loop and
// the tile walk are that file's).  A segment's UNITS are the 16-byte-aligned words of DESTINATION memory it touches; the units of all
// segments, one after the other, are cut into tiles of kTileUnits (BROTLI_AMD_UNSHUFFLE_TILE_BYTES of destination), and the blocks take the
// tiles in turns.  A lane finds the segment of a unit by a binary search in the prefix sum of the segments' unit counts, which every block
// builds in LDS for kChunkSegs segments at a time; a tile that lies inside one segment -- every tile of a long one -- is searched for once,
// and its width is then the same for every lane, so the unit's code is chosen once per tile.
//
// A lane produces one word: w runs of 16 / w (+ 1) plane bytes, each loaded as the aligned dwords around it.  Neighbouring lanes read
// neighbouring runs of the same plane, so a wave's load instruction reads one contiguous stretch of 64 x 16 / w bytes of a plane.  Width 8,
// whose runs would be two bytes, takes two neighbouring words a lane in a tile that lies inside one segment.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "brotli_device_abi.h"
#include "brotli_unshuffle.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kUnitsPerThread = 4;
constexpr uint32_t kTileUnits = kThreads * kUnitsPerThread;
constexpr uint32_t kChunkSegs = kThreads * 4;   // segments whose prefix sum lies in LDS at a time: four a thread

static_assert(kTileUnits * 16u == BROTLI_AMD_UNSHUFFLE_TILE_BYTES, "the tile the header names");

// the units [lo, hi) of the tile at t0 that are this thread's, all of one segment of width W whose first unit is `first`.  Width 8: two neighbouring
// units a time (brotli_unshuffle.h: brotli_amd_unshuffle_two_units_w), so that a plane's run is four bytes, not two
template <uint32_t W>
__device__ __forceinline__ void tile_of_one(const BrotliAmdUnshuffleSeg& sg, uint64_t first, uint64_t t0, uint64_t lo, uint64_t hi, uint32_t tid) {
  const uint64_t src = (uint64_t)(uintptr_t)sg.src, dst = (uint64_t)(uintptr_t)sg.dst;
  if constexpr (W == 8u) {
#pragma unroll
    for (uint32_t it = 0; it < kUnitsPerThread / 2u; it++) {
      const uint64_t g = t0 + 2u * (it * kThreads + tid);
      if (g >= lo && g + 1u < hi) brotli_amd_unshuffle_two_units_w<W>(src, dst, sg.len, g - first, hi - first);
      else if (g >= lo && g < hi) brotli_amd_unshuffle_unit_w<W>(src, dst, sg.len, g - first);
      else if (g + 1u >= lo && g + 1u < hi) brotli_amd_unshuffle_unit_w<W>(src, dst, sg.len, g + 1u - first);
    }
  } else {
#pragma unroll
    for (uint32_t it = 0; it < kUnitsPerThread; it++) {
      const uint64_t g = t0 + it * kThreads + tid;
      if (g >= lo && g < hi) brotli_amd_unshuffle_unit_w<W>(src, dst, sg.len, g - first);
    }
  }
}

// This block's tiles among the units [base, end) of one chunk of segments (pre[]: the units in front of each, segs: the chunk's first): every thread
// of the block makes the same walk and produces its own units.  -> the block's next tile (one that goes on behind `end` stays the block's).
__device__ __forceinline__ uint64_t take_tiles(const uint64_t* pre, const BrotliAmdUnshuffleSeg* segs, uint64_t base, uint64_t end, uint64_t tile,
                                               uint32_t grid, uint32_t tid) {
  while (tile * kTileUnits < end) {
    const uint64_t t0 = tile * kTileUnits, t1 = t0 + kTileUnits;
    const uint64_t lo = t0 > base ? t0 : base, hi = t1 < end ? t1 : end;   // the tile's units among this chunk's segments
    if (lo < hi) {   // (not: a tile that began in the chunk before, and this chunk has no units)
      const uint32_t ja = brotli_amd_unshuffle_find_seg(pre, kChunkSegs, lo), jb = brotli_amd_unshuffle_find_seg(pre, kChunkSegs, hi - 1u);
      if (ja == jb) {   // one segment's: the rule for a long one
        const BrotliAmdUnshuffleSeg sg = segs[ja];
        const uint64_t first = pre[ja];
        switch (sg.width) {
          case 1u: tile_of_one<1u>(sg, first, t0, lo, hi, tid); break;
          case 2u: tile_of_one<2u>(sg, first, t0, lo, hi, tid); break;
          case 4u: tile_of_one<4u>(sg, first, t0, lo, hi, tid); break;
          case 8u: tile_of_one<8u>(sg, first, t0, lo, hi, tid); break;
          default: break;   // (the host lets no other width through)
        }
      } else {
        for (uint32_t it = 0; it < kUnitsPerThread; it++) {
          const uint64_t g = t0 + it * kThreads + tid;
          if (g >= lo && g < hi) {
            const uint32_t j = brotli_amd_unshuffle_find_seg(pre, kChunkSegs, g);
            const BrotliAmdUnshuffleSeg sg = segs[j];
            brotli_amd_unshuffle_unit((uint64_t)(uintptr_t)sg.src, (uint64_t)(uintptr_t)sg.dst, sg.len, sg.width, g - pre[j]);
          }
        }
      }
    }
    if (t1 > end) break;   // (the tile goes on in the next chunk's segments)
    tile += grid;
  }
  return tile;
}

__global__ __launch_bounds__(kThreads) void brotli_amd_unshuffle_kernel(const BrotliAmdUnshuffleSeg* __restrict__ segs, uint32_t n) {
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
      u[k] = j < cnt ? brotli_amd_unshuffle_seg_units((uint64_t)(uintptr_t)segs[c0 + j].dst, segs[c0 + j].len) : 0u;
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

extern "C" uint32_t brotli_amd_unshuffle_tile_bytes(void) { return BROTLI_AMD_UNSHUFFLE_TILE_BYTES; }

// units: the units of all segments together (brotli_amd_unshuffle_seg_units: the host has the table) -- a launch of a few short segments has a
// few blocks, not a device full of blocks that find nothing to do
extern "C" hipError_t brotli_amd_launch_unshuffle(const BrotliAmdUnshuffleSeg* d_segs, uint32_t n, uint64_t units, hipStream_t stream) {
  if (n == 0u || units == 0u) return hipSuccess;
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  // four blocks of four waves a CU, and no more blocks than there are tiles
  const uint64_t grid = std::min<uint64_t>((uint64_t)(cus > 0 ? cus : 1) * 4u, (units + kTileUnits - 1u) / kTileUnits);
  hipLaunchKernelGGL(brotli_amd_unshuffle_kernel, dim3((uint32_t)grid), dim3(kThreads), 0, stream, d_segs, n);
  return hipGetLastError();
}
